"""The memory contract of icpflow_seq_bucket_table, in the style of tests/test_gpu_classes_workspace_contract.py: "the caller
owns the memory".  It runs on EXACTLY its *_workspace_bytes() bytes -- the documented formula, asserted here, not recorded
numbers --, filled with a poison, between two guards in the same allocation, its table and info between guards as well;
asserted: status 0, every guard byte intact, the output bit-identical to an ordinary run, one byte too few refused with
ICPFLOW_E_WORKSPACE before anything is written, the same result on a workspace that is 8- but not 256-byte aligned, and a
workspace that is not 8-byte aligned refused.

Who initialises what (csrc/bucketeval.hip): every workgroup zeroes its table in LDS and stores its whole partial -- G * S * 3 + 2
words -- whatever it saw, and the second kernel reads exactly the partials of the grid that was launched; nothing in the
workspace is read before it is written."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import argo_restatement as ar         # noqa: E402
import bucket_restatement as br       # noqa: E402
import class_restatement as cr        # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 16
GUARD_BYTE = 0x5C
DEV = torch.device("cuda:0")
G, S = 33, 51
WORDS = G * S * 3


def _guarded(nbytes, poison):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _inputs():
    """the f64 fixture's sample five times over, so that the grid has more than one workgroup (5 035 rows: three)"""
    s, pred = cr.fixture_sample("g15_argo_f64")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([a] * 5).astype(dt))).to(DEV)   # noqa: E731
    return dict(pts=up(s["raw_points"], np.float64), tim=up(s["time_indice"], np.int32), cls=up(s["classes"], np.float64),
                gt=up(s["scene_flow"], np.float64), pred=up(pred, np.float32), m=5 * len(pred), s=s, host_pred=pred)


def _run(x, poison=None, shift=0, expect_unaligned=False):
    """-> the table's and info's bytes; guarded and poisoned when `poison` is given; the workspace `shift` bytes further on"""
    from icp_flow_amd import _lib
    L, st, p = _lib._L, _lib.stream(DEV), _lib.ptr
    m = x["m"]
    need = L.icpflow_seq_bucket_table_workspace_bytes(m, G, S)
    # exact size: a workgroup per 2048 rows (256 at most), G * S * 3 + 2 words each; a 256-byte multiple
    grid = min(max(-(-m // 2048), 1), 256)
    assert grid == 3 and need == -(-grid * (WORDS + 2) * 8 // 256) * 256
    sizes = dict(ws=need + shift, table=(WORDS + 2) * 8)
    if poison is None:
        bufs = {k: torch.zeros(v, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    vp = lambda k, off=0: ctypes.c_void_p(at[k] + off)   # noqa: E731
    sp = np.asarray(br.EDGES, np.float64)
    args = lambda nbytes: (p(x["pts"]), p(x["tim"]), p(x["cls"]), p(x["gt"]), p(x["pred"]), m, 2, _lib.SEQ_CROP_XYZ, 32.0, 32.0, 0.3, -1.0,   # noqa: E731
                           G, sp.ctypes.data_as(ctypes.c_void_p), S, vp("table"), vp("table", WORDS * 8), vp("ws", shift),
                           ctypes.c_size_t(nbytes), st)
    before = {k: b.clone() for k, b in bufs.items()}
    if expect_unaligned:
        assert L.icpflow_seq_bucket_table(*args(need)) == -1 and b"8-byte aligned" in L.icpflow_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)
        return None
    if poison is not None:
        # one byte too few: refused before anything is written
        assert L.icpflow_seq_bucket_table(*args(need - 1)) == -2 and b"workspace" in L.icpflow_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    _lib.call("icpflow_seq_bucket_table", *args(need))
    torch.cuda.synchronize()
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
    return (bufs["table"] if poison is None else bufs["table"][GUARD: GUARD + sizes["table"]]).clone()


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_runs_on_exactly_its_bytes_whatever_they_held(poison):
    x = _inputs()
    want = _run(x)
    got = _run(x, poison)
    assert torch.equal(want, got)
    words = want.view(torch.int64).cpu().numpy()
    one = br.table(ar.setting_args("default"), x["s"], x["host_pred"], x["s"]["classes"])
    counts = words[:WORDS].reshape(G, S, 3)[:, :, 0]
    assert np.array_equal(counts, 5 * one.counts) and int(counts.sum()) > 0
    assert (int(words[WORDS]), int(words[WORDS + 1])) == (5 * one.kept0, 0)


def test_workspace_at_base_plus_8():
    """a workspace that is 8- but not 256-byte aligned: the partials are addressed relative to the base, the result is the
    same; base + 4 is refused with nothing written"""
    x = _inputs()
    assert torch.equal(_run(x), _run(x, 0xA5, shift=8))
    _run(x, 0xA5, shift=4, expect_unaligned=True)

"""The memory contract of icpflow_seq_segment_table, in the style of tests/test_gpu_seqeval_workspace_contract.py: "the caller
owns the memory".  The call runs on EXACTLY its *_workspace_bytes() bytes, filled with a poison, between two guards in the same
allocation, its outputs between guards as well; asserted: status 0, every guard byte intact, the outputs bit-identical to an
ordinary run, one byte too few refused with ICPFLOW_E_WORKSPACE before anything is written, and the same result on a workspace
that starts 16 bytes behind a 256-byte boundary.

Who initialises what (csrc/segeval.hip): the order is written for every row by table.hip's scatter, the (label, count, start)
rows and the chunk starts for every segment, and every chunk's workgroup stores its whole partial; the final kernel reads
exactly the chunks of the segments it writes.  Nothing in the workspace is read before it is written."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_restatement as sg      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 16
GUARD_BYTE = 0x5C
DEV = torch.device("cuda:0")
LMAX = 32


def _guarded(nbytes, poison):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _inputs():
    g = sg.load("g14_segments_f64")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(DEV)   # noqa: E731
    return dict(pts=up(g["src_points"], np.float64), lab=up(g["src_labels"], np.float32), gt=up(g["flow_gt"], np.float64),
                pred=up(g["flow_pd"], np.float32), n=len(g["src_points"]), z_min=float(g["z_min"]))


def _run(x, poison=None, shift=0):
    """-> (table bytes, num bytes); guarded and poisoned when `poison` is given; the workspace `shift` bytes further on"""
    from icp_flow_amd import _lib
    L, st, p = _lib._L, _lib.stream(DEV), _lib.ptr
    n = x["n"]
    need = L.icpflow_seq_segment_table_workspace_bytes(n, LMAX)
    # exact size: the carve of csrc/segeval.hip (tests/test_segments.py::_expected_workspace spells it out)
    al = lambda b: -(-b // 256) * 256   # noqa: E731
    chunks = n // sg.CHUNK + min(n, LMAX) + 1
    assert need == (al(n * 8) + al(LMAX * 72) + al((LMAX + 1) * 4) + al(chunks * 96)
                    + al(4 * al(LMAX * 4) + al(n * 2) + al(-(-n // 512) * LMAX * 4)))
    sizes = dict(ws=need + shift, table=LMAX * 16 * 8, num=4)
    if poison is None:
        bufs = {k: torch.zeros(v, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    vp = lambda k, off=0: ctypes.c_void_p(at[k] + off)   # noqa: E731
    args = lambda nbytes: (p(x["pts"]), p(x["lab"]), n, p(x["gt"]), p(x["pred"]), x["z_min"], vp("table"), LMAX, vp("num"),   # noqa: E731
                           vp("ws", shift), ctypes.c_size_t(nbytes), st)
    if poison is not None:
        before = {k: b.clone() for k, b in bufs.items()}
        assert L.icpflow_seq_segment_table(*args(need - 1)) == -2 and b"workspace" in L.icpflow_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    _lib.call("icpflow_seq_segment_table", *args(need))
    torch.cuda.synchronize()
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
    view = lambda k: (bufs[k] if poison is None else bufs[k][GUARD: GUARD + sizes[k]]).clone()   # noqa: E731
    return view("table"), view("num")


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_runs_on_exactly_its_bytes_whatever_they_held(poison):
    x = _inputs()
    want = _run(x)
    got = _run(x, poison)
    num = int(want[1].view(torch.int32)[0])
    assert num == 14 and torch.equal(got[1], want[1])
    # (rows from num on are not written: they keep what the buffer held)
    assert torch.equal(got[0][: num * 128], want[0][: num * 128]) and bool((got[0][num * 128:] == poison).all())
    table = want[0].view(torch.float64).cpu().numpy().reshape(LMAX, 16)[:num]
    ref, _, absx, absm = sg.table_numpy(x["pts"].cpu().numpy(), x["lab"].cpu().numpy(), x["pred"].cpu().numpy(), x["gt"].cpu().numpy(), x["z_min"])
    sg.check_table(table, ref, absx, absm)


def test_workspace_at_base_plus_16():
    """a workspace that is 8- but not 256-byte aligned: every region is carved relative to the base, the result is the same"""
    x = _inputs()
    want = _run(x)
    got = _run(x, 0xA5, shift=16)
    num = int(want[1].view(torch.int32)[0])
    assert torch.equal(got[1], want[1]) and torch.equal(got[0][: num * 128], want[0][: num * 128])

"""The memory contract of icpflow_seq_gt_flow and icpflow_seq_metrics, in the style of tests/test_gpu_ego_workspace_contract.py:
"the caller owns the memory".  Both run on EXACTLY their *_workspace_bytes() bytes, filled with a poison, between two guards
in the same allocation, their outputs between guards as well; asserted: status 0, every guard byte intact, every output
bit-identical to an ordinary run, and one byte too few refused with ICPFLOW_E_WORKSPACE before anything is written.

Who initialises what (csrc/seqeval.hip): every workgroup stores its whole partial -- (F - 1) * 36 + 2 words for the table, one
word for the flow's count of refused rows -- whatever it saw, and the final kernels read exactly the partials of the grid that
was launched; nothing in the workspace is read before it is written."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqeval_restatement as sr      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 16
GUARD_BYTE = 0x5C
DEV = torch.device("cuda:0")


def _guarded(nbytes, poison):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _inputs():
    g = sr.load("g13_seqeval_f5_f64")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(DEV)   # noqa: E731
    return dict(pts=up(g["raw_points"], np.float64), tim=up(g["time_indice"], np.int32), inst=up(g["inst_labels"], np.int32),
                sd=up(np.where(np.isin(g["sd_labels"], (0, 1)), g["sd_labels"], 2), np.int32),
                fb=up(np.where(np.isin(g["fb_labels"], (0, 1)), g["fb_labels"], 2), np.int32), ego=up(g["ego_motion_gt"], np.float64),
                tsfm=up(g["bbox_tsfm"], np.float64), gt=up(g["scene_flow"], np.float64), pred=up(g["pred_flow"], np.float32),
                m=len(g["raw_points"]), F=int(g["num_frames"]), K=g["bbox_tsfm"].shape[0])


def _run(x, poison=None):
    """-> (flow bytes, refused rows, table + info bytes); guarded and poisoned when `poison` is given"""
    from icp_flow_amd import _lib
    L, st, p = _lib._L, _lib.stream(DEV), _lib.ptr
    m, F, K = x["m"], x["F"], x["K"]
    need_flow, need_tab = L.icpflow_seq_gt_flow_workspace_bytes(m), L.icpflow_seq_metrics_workspace_bytes(m, F)
    # exact sizes: a workgroup per 2048 rows (256 at most); one word each for the flow, (F - 1) * 36 + 2 for the table; 256-byte multiples
    G = min(max(-(-m // 2048), 1), 256)
    assert need_flow == -(-G * 8 // 256) * 256 and need_tab == -(-G * ((F - 1) * 36 + 2) * 8 // 256) * 256
    sizes = dict(ws_flow=need_flow, ws_tab=need_tab, flow=m * 24, bad=8, table=(F * 36 + 2) * 8)
    if poison is None:
        bufs = {k: torch.zeros(v, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    vp = lambda k, off=0: ctypes.c_void_p(at[k] + off)   # noqa: E731
    flow_args = lambda nbytes: (p(x["pts"]), p(x["tim"]), p(x["inst"]), m, p(x["ego"]), F, p(x["tsfm"]), K, _lib.SEQ_OUT_FLOW,   # noqa: E731
                                vp("flow"), vp("bad"), vp("ws_flow"), ctypes.c_size_t(nbytes), st)
    tab_args = lambda nbytes: (p(x["pts"]), p(x["tim"]), p(x["sd"]), p(x["fb"]), p(x["gt"]), p(x["pred"]), m, F, _lib.SEQ_CROP_XYZ,   # noqa: E731
                               32.0, 32.0, 0.3, vp("table"), vp("table", F * 36 * 8), vp("ws_tab"), ctypes.c_size_t(nbytes), st)
    if poison is not None:
        # one byte too few: refused before anything is written
        before = {k: b.clone() for k, b in bufs.items()}
        assert L.icpflow_seq_gt_flow(*flow_args(need_flow - 1)) == -2 and b"workspace" in L.icpflow_last_error()
        assert L.icpflow_seq_metrics(*tab_args(need_tab - 1)) == -2 and b"workspace" in L.icpflow_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    _lib.call("icpflow_seq_gt_flow", *flow_args(need_flow))
    _lib.call("icpflow_seq_metrics", *tab_args(need_tab))
    torch.cuda.synchronize()
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
    view = lambda k: (bufs[k] if poison is None else bufs[k][GUARD: GUARD + sizes[k]]).clone()   # noqa: E731
    return view("flow"), view("bad"), view("table")


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_both_run_on_exactly_their_bytes_whatever_they_held(poison):
    x = _inputs()
    want = _run(x)
    got = _run(x, poison)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert int(want[1].view(torch.int64)[0]) == 0 and int(want[2].view(torch.int64)[36]) > 0
    g = sr.load("g13_seqeval_f5_f64")
    assert np.abs(want[0].view(torch.float64).cpu().numpy().reshape(-1, 3) - g["scene_flow"]).max() <= sr.gt_flow_bound(
        g["raw_points"], g["ego_motion_gt"], g["bbox_tsfm"])

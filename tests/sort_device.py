"""Device helper of tests/test_gpu_sorts.py: one raw C-ABI call of a fused entry point on an exactly sized workspace filled with a
NaN poison (every byte 0xFF: a NaN as a float, -1 as an int), then the arrays its sorts left there, read by the offsets of
icpflow_selftest_workspace_layout.  Which call leaves which array alone (csrc/api.hip):

  init_pose   icpflow_estimate_init_pose: the vote's sort (zsortA / zsortC / voteKey) and, for N > 2048, the axis sort for the
              scoring sweeps (no swap flags: the src cloud moves; no direction keys: the entry never asks for them)
  hist_icp    icpflow_hist_icp with max_iterations = 1: lengths, swap, both sorts; the ICP and the roll-back check read the
              sorted clouds and write none of them
  apply_icp   icpflow_apply_icp with max_iterations = 1: the axis sort with the initial poses as the pre-pose, no boxes
  icp         icpflow_icp with max_iterations = 1 and a NULL pre-pose (moving image only as rows: no sortXsoa)
"""
import contextlib
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

from icp_flow_amd import _lib

DEV = torch.device("cuda:0")
POISON_WORD = 0xFFFFFFFF
LAYOUT = ["lenA", "lenC", "swap", "pts", "sortX", "sortYsoa", "sortXsoa", "axis", "zsortA", "zsortC", "voteKey"]
F = np.float32


def edges(tf=2.0, th=0.1, ez=None):
    """left bin edges of the vote box (the layout of utils_hist.bin_edges); ez: other z edges"""
    ex = np.arange(-tf, tf + th - 1e-8, th, dtype=F)
    ez = np.arange(-th, 2 * th - 1e-8, th, dtype=F) if ez is None else np.asarray(ez, F)
    return ex, ex.copy(), ez


def layout(B, N, lens):
    off = (ctypes.c_size_t * len(LAYOUT))()
    rc = _lib._L.icpflow_selftest_workspace_layout(B, N, lens[0], lens[1], lens[2], off, len(LAYOUT))
    assert rc == 0, _lib._L.icpflow_last_error()
    return dict(zip(LAYOUT, [int(o) for o in off]))


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(entry, S, D, init=None, ez=None, stream=None, **switches):
    """-> the arrays of LAYOUT as NumPy arrays (raw bits: float arrays as float32, ids still in w), plus B, N, NP16, h_box"""
    B, N, _ = S.shape
    ex, ey, ez_ = edges(ez=ez)
    lens = (len(ex), len(ey), len(ez_)) if entry in ("init_pose", "hist_icp") else (0, 0, 0)
    need = _lib.workspace_bytes(B, N, lens)
    P = _lib.ptr
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        s, d = G(S), G(D)
        gx, gy, gz = G(ex), G(ey), G(ez_)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        ws.fill_(0xFF)
        T = torch.zeros((B, 4, 4), dtype=torch.float32, device=DEV)
        it = torch.zeros(2, dtype=torch.int32, device=DEV)
        keep = [s, d, gx, gy, gz, ws, T, it]
        with _lib.options(**switches):
            st, o = _lib.stream(DEV), _lib.opt()
            if entry == "init_pose":
                rc = _lib._L.icpflow_estimate_init_pose(P(s), P(d), B, N, P(gx), lens[0], P(gy), lens[1], P(gz), lens[2], 0.0, P(T), P(ws), need, st, o)
            elif entry == "hist_icp":
                rc = _lib._L.icpflow_hist_icp(P(s), P(d), B, N, P(gx), lens[0], P(gy), lens[1], P(gz), lens[2], 0.0, 0.1, 1, 1e-6, 0, P(T),
                                              P(it), P(ws), need, st, o)
            elif entry == "apply_icp":
                gi = G(np.asarray(init, F))
                keep.append(gi)
                rc = _lib._L.icpflow_apply_icp(P(s), P(d), P(gi), B, N, 0.1, 1, 1e-6, 0, P(T), P(it), P(ws), need, st, o)
            elif entry == "icp":
                R = torch.zeros((B, 3, 3), dtype=torch.float32, device=DEV)
                t = torch.zeros((B, 3), dtype=torch.float32, device=DEV)
                rm = torch.zeros(B, dtype=torch.float32, device=DEV)
                keep += [R, t, rm]
                rc = _lib._L.icpflow_icp(P(s), P(d), None, B, N, 0.1, 1, 1e-6, 0, P(R), P(t), P(rm), P(it[0:1]), P(it[1:2]), P(ws), need, st, o)
            else:
                raise ValueError(entry)
        assert rc == 0, (rc, _lib._L.icpflow_last_error())
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    off = layout(B, N, lens)
    NP16 = (N + 15) // 16 * 16

    def take(name, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return raw[off[name]:off[name] + n].view(dtype).reshape(shape).copy()

    return SimpleNamespace(
        B=B, N=N, NP16=NP16, h_box=ez_[-1] - ez_[0], entry=entry,
        lenA=take("lenA", np.int32, B), lenC=take("lenC", np.int32, B), swap=take("swap", np.uint8, B),
        pts=take("pts", F, B, N, 4), sortX=take("sortX", F, B, N, 4), sortYsoa=take("sortYsoa", F, B, 3, NP16),
        sortXsoa=take("sortXsoa", F, B, 3, NP16), axis=take("axis", np.int32, B), zsortA=take("zsortA", F, B, N, 4),
        zsortC=take("zsortC", F, B, N, 4), voteKey=take("voteKey", F, B, 8))


def poisoned(a):
    """a word of the poison is left in the array"""
    return bool((np.ascontiguousarray(a).view(np.uint32) == POISON_WORD).any()) if a.dtype.itemsize == 4 else bool((a == 0xFF).any())

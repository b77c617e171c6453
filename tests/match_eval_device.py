"""What the GPU tests of icpflow_match_eval share, in the style of tests/trust_device.py: the raw call on buffers the test owns -- a
workspace of EXACTLY the size the library asks for, filled with 0xFF (NaN floats, -1 integers), between two guards, and each of the
six outputs between two guards in an allocation of its own, poisoned beforehand -- and the comparison with
tests/match_eval_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_eval_restatement as mr      # noqa: E402
import residual_device as rd             # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, OUT_POISON = 0xFF, 0xA5
OUTPUTS = (("errors", 2), ("inliers", 2), ("ratios", 2), ("ious", 2), ("translations", 3), ("rotations", 3))


def run(case, no_eval_sweep=False, stream=None):
    """One call of icpflow_match_eval on `case` (dict P1, P2 [B, N, 4], T [B, 4, 4], thres) -> dict of float32 arrays [B, 2] / [B, 3].
    Status 0, the guards of the workspace and of every output intact, every output word written."""
    from icp_flow_amd import _lib
    L, ptr = _lib._L, _lib.ptr
    P1, P2, T = upload(case["P1"], F), upload(case["P2"], F), upload(case["T"], F)
    B, N = int(P1.shape[0]), int(P1.shape[1])
    need = _lib.workspace_bytes(B, N)
    ws = rd._guarded(need, WS_POISON)
    sizes = {k: B * c * 4 for k, c in OUTPUTS}
    bufs = {k: rd._guarded(v, OUT_POISON) for k, v in sizes.items()}
    at = lambda b: ctypes.c_void_p(b.data_ptr() + GUARD)   # noqa: E731
    torch.cuda.synchronize()                                # (the uploads and the poison ran on the default stream)
    with _lib.options(no_eval_sweep=bool(no_eval_sweep)), torch.cuda.stream(stream):
        rc = L.icpflow_match_eval(ptr(P1), ptr(P2), ptr(T), B, N, float(case["thres"]), *[at(bufs[k]) for k, _ in OUTPUTS],
                                  at(ws), need, _lib.stream(DEV), _lib.opt())
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out = {}
    for k, c in OUTPUTS:
        assert rd._guards_intact(bufs[k], sizes[k]), f"guard of {k} changed"
        words = bufs[k][GUARD: GUARD + sizes[k]].clone().view(torch.int32).cpu().numpy()
        out[k] = words.view(F).reshape(B, c)
        # (0xA5A5A5A5 is an ordinary negative float32, -2.87e-16: no result of these cases)
        assert not (words.view(np.uint32) == np.uint32(0xA5A5A5A5)).any(), f"{k}: words left unwritten"
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k, _ in OUTPUTS)


def compare(got, recs, want, poses, rot_bound, label=""):
    """The call against the restatement.  inliers, ratios, ious: array_equal (NaN in the same places).  errors and translations:
    inside the interval the summation order allows (match_eval_restatement.sum_bounds).  rotations: within rot_bound degrees of
    the float64 evaluation of the same float32 entries, NaN where that is NaN.  -> (error values not bit-equal to the restatement's,
    the largest rotation difference in degrees)"""
    for k in ("inliers", "ratios", "ious"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (label, k, np.argwhere(~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k]))))[:8])
    unequal, worst = 0, 0.0
    for b, r in enumerate(recs):
        for d, n in ((0, r["n1"]), (1, r["n2"])):
            lo, hi = mr.sum_bounds(r["S"][d], r["S"][d], n)
            g = got["errors"][b, d]
            ok = (np.isnan(lo) and np.isnan(g)) or (lo <= g <= hi)
            assert ok, (label, "errors", b, d, float(g), float(lo), float(hi), n)
            unequal += int(F(g).view(np.uint32) != F(want["errors"][b, d]).view(np.uint32))
        lo, hi = mr.translation_bounds(r)
        g = got["translations"][b]
        ok = (np.isnan(lo) & np.isnan(g)) | ((lo <= g) & (g <= hi))
        assert ok.all(), (label, "translations", b, g, lo, hi)
        ref = mr.rotations64(poses[b])
        g = got["rotations"][b].astype(np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(ref)), (label, "rotations: NaN", b, g, ref)
        diff = np.abs(g - ref)[~np.isnan(ref)]
        if diff.size:
            worst = max(worst, float(diff.max()))
        assert (diff <= rot_bound).all(), (label, "rotations", b, g, ref)
    return unequal, worst

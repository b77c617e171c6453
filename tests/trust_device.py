"""What the GPU tests of icpflow_flow_trust share, in the style of tests/sight_device.py: one call on buffers the test owns --
every output between two guards in its own allocation, poisoned beforehand; the tables uploaded at [Lmax] rows with NaN from
the segments' number on -- and the comparison, array_equal throughout, with tests/trust_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd                  # noqa: E402
import trust_restatement as T                 # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
POISON = 0xA5


def _padded(table, cols, Lmax):
    """a segment table as the device holds it: [Lmax][cols], the rows no call wrote full of NaN"""
    if table is None:
        return None
    t = np.full((Lmax, cols), np.nan)
    rows = np.asarray(table, np.float64).reshape(-1, cols)[:Lmax]
    t[:len(rows)] = rows
    return upload(t, np.float64)


def run(case, Lmax=None, num=None, params=None, expect=0, expect_message=None, spoil=None, stream=None):
    """One call.  case: dict(after, flow, labels, d2, code, resid, sight, pairs) of numpy arrays (flow, code, sight, pairs may be
    None).  num: *d_num (default: the residual table's rows); Lmax: default max(num, 1).  spoil: arguments replaced just before the
    call (name -> value).  expect 0: status 0 asserted, the guards intact, d_segment from *d_num on untouched
    -> dict(trust uint8 [n], segment uint8 [L], counts int64 [16]).  expect != 0: that status and message asserted, every byte of
    every output as it was."""
    from icp_flow_amd import _lib
    L, ptr = _lib._L, _lib.ptr
    resid = np.asarray(case["resid"], np.float64).reshape(-1, 18)
    num = len(resid) if num is None else int(num)
    Lmax = max(len(resid), 1) if Lmax is None else int(Lmax)
    after = upload(np.asarray(case["after"], F).reshape(-1, 3), F)
    n = after.shape[0]
    flow = None if case.get("flow") is None else upload(np.asarray(case["flow"], F).reshape(-1, 3), F)
    labels, d2 = upload(np.asarray(case["labels"], F).reshape(-1), F), upload(np.asarray(case["d2"], F).reshape(-1), F)
    code = None if case.get("code") is None else upload(np.asarray(case["code"]).reshape(-1), np.int32)
    pairs = None if case.get("pairs") is None or len(case["pairs"]) == 0 else upload(np.asarray(case["pairs"], F), F)
    P, stride = (0, 1) if pairs is None else (int(pairs.shape[0]), int(pairs.shape[1]))
    a = dict(after=ptr(after), flow=ptr(flow), labels=ptr(labels), n=n, resid=ptr(_keep(_padded(resid, 18, max(Lmax, 1)))),
             sight=ptr(_keep(_padded(case.get("sight"), 24, max(Lmax, 1)))), num=ptr(_keep(upload(np.array([num]), np.int32))), Lmax=Lmax, d2=ptr(d2),
             code=ptr(code), pairs=ptr(pairs), P=P, stride=stride)
    a.update(spoil or {})
    p = params if isinstance(params, _lib.TrustParams) else _lib.TrustParams.defaults(**(params or {}))
    sizes = dict(trust=n, segment=max(Lmax, 1), counts=128)
    bufs = {k: rd._guarded(v, POISON) for k, v in sizes.items()}
    at = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + GUARD)   # noqa: E731
    held = {k: v.clone() for k, v in bufs.items()}
    torch.cuda.synchronize()                       # (the uploads and the poison ran on the default stream)
    with torch.cuda.stream(stream):                # (None: the current stream)
        rc = L.icpflow_flow_trust(a["after"], a["flow"], a["labels"], a["n"], a["resid"], a["sight"], a["num"], a["Lmax"], a["d2"], a["code"],
                                  a["pairs"], a["P"], a["stride"], ctypes.byref(p), a.get("trust", at("trust")), a.get("segment", at("segment")),
                                  a.get("counts", at("counts")), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    _KEPT.clear()
    assert rc == expect, (rc, msg)
    if expect != 0:
        assert expect_message is None or expect_message in msg, msg
        assert all(torch.equal(bufs[k], held[k]) for k in bufs), "a refused call wrote something"
        return None
    for k, v in bufs.items():
        assert rd._guards_intact(v, sizes[k]), f"guard of {k} changed"
    inner = lambda k, dt: bufs[k][GUARD: GUARD + sizes[k]].clone().view(dt).cpu().numpy()   # noqa: E731
    written = T.segments_of(num, Lmax)
    assert torch.equal(bufs["segment"][GUARD + written:], held["segment"][GUARD + written:]), "d_segment from *d_num on was written"
    return dict(trust=inner("trust", torch.uint8), segment=inner("segment", torch.uint8)[:written], counts=inner("counts", torch.int64))


_KEPT = []


def _keep(t):
    """(an uploaded tensor that only a pointer refers to stays alive until the call is through)"""
    _KEPT.append(t)
    return t


def want(case, Lmax=None, num=None, params=None):
    """the restatement's answer to the same call"""
    resid = np.asarray(case["resid"], np.float64).reshape(-1, 18)
    num = len(resid) if num is None else int(num)
    Lmax = max(len(resid), 1) if Lmax is None else int(Lmax)
    padded = np.full((Lmax, 18), np.nan)
    padded[:min(len(resid), Lmax)] = resid[:Lmax]
    sight = None
    if case.get("sight") is not None:
        sight = np.full((Lmax, 24), np.nan)
        sight[:min(len(resid), Lmax)] = np.asarray(case["sight"], np.float64).reshape(-1, 24)[:Lmax]
    pairs = case.get("pairs")
    pl = np.zeros(0, F) if pairs is None or len(pairs) == 0 else np.asarray(pairs, F)[:, 0]
    return T.trust(case["after"], case.get("flow"), case["labels"], padded, sight, num, case["d2"], case.get("code"), pl, **(params or {}))


def check(case, label="", **kw):
    """the call against the restatement, array_equal.  -> (the call's dict, the restatement's)"""
    got = run(case, **{k: v for k, v in kw.items() if k in ("Lmax", "num", "params", "stream")})
    exp = want(case, **{k: v for k, v in kw.items() if k in ("Lmax", "num", "params")})
    assert np.array_equal(got["segment"], exp["segment"]), (label, "segment", np.flatnonzero(got["segment"] != exp["segment"])[:8])
    assert np.array_equal(got["trust"], exp["trust"]), (label, "trust", np.flatnonzero(got["trust"] != exp["trust"])[:8])
    assert np.array_equal(got["counts"], exp["counts"]), (label, "counts", got["counts"], exp["counts"])
    return got, exp

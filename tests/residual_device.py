"""What the GPU tests of icpflow_nn_residual share: one call on buffers the test owns -- every output between two guards in its
own allocation, filled with a poison beforehand, the workspace of EXACTLY the size the library asks for, poisoned and guarded
too -- and the comparison with tests/residual_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_restatement as rr        # noqa: E402

GUARD = 4096
GUARD_BYTE = 0x5C
DEV = torch.device("cuda:0")
OUTPUTS = ("d2", "idx", "table")


def _guarded(nbytes, poison):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def upload(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def run(query, target, flow=None, radius=2.0, groups=None, G=1, edges=(), outputs=OUTPUTS, poison=0xA5, shift=0, short=0, expect=0,
        expect_message=None):
    """One call on the current stream.  expect 0: status 0 asserted, every guard intact -> dict(d2 float32 [n], idx int32 [n],
    words int64 [G * (E + 4)], info int64 [4]; None for an output not asked for).  expect != 0: that status (and
    `expect_message` in the message) asserted, and every byte of every buffer as it was.  shift: the workspace that many bytes
    further on; short: that many bytes fewer than the library asks for."""
    from icp_flow_amd import _lib
    L, p = _lib._L, _lib.ptr
    q, t = upload(np.asarray(query, np.float32).reshape(-1, 3), np.float32), upload(np.asarray(target, np.float32).reshape(-1, 3), np.float32)
    f = None if flow is None else upload(np.asarray(flow, np.float32).reshape(-1, 3), np.float32)
    g = None if groups is None else upload(np.asarray(groups).reshape(-1), np.int32)
    n, m, E = q.shape[0], t.shape[0], len(edges)
    ed = np.ascontiguousarray(edges, dtype=np.float64)
    need = int(L.icpflow_nn_residual_workspace_bytes(n, m, G, E))
    words = max(G, 0) * (max(E, 0) + 4)
    sizes = dict(d2=4 * n, idx=4 * n, table=8 * words, info=32, ws=max(need, 16) + shift)
    bufs = {k: _guarded(v, poison) for k, v in sizes.items()}
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].data_ptr() + GUARD + off)   # noqa: E731
    before = {k: b.clone() for k, b in bufs.items()}
    rc = L.icpflow_nn_residual(p(q), p(f), n, p(t), m, float(radius), p(g), G, ed.ctypes.data_as(ctypes.c_void_p) if E else None, E,
                               at("d2") if "d2" in outputs else None, at("idx") if "idx" in outputs else None,
                               at("table") if "table" in outputs else None, at("info"), at("ws", shift), ctypes.c_size_t(need - short),
                               _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == expect, (rc, msg)
    if expect != 0:
        assert expect_message is None or expect_message in msg, msg
        assert all(torch.equal(bufs[k], before[k]) for k in bufs), "a refused call wrote something"
        return None
    for k, b in bufs.items():
        assert _guards_intact(b, sizes[k]), f"guard of {k} changed"
    inner = lambda k, dt: bufs[k][GUARD: GUARD + sizes[k]].clone().view(dt).cpu().numpy()   # noqa: E731
    for k in OUTPUTS:                              # an output not asked for is not written
        if k not in outputs:
            assert torch.equal(bufs[k], before[k]), k
    return dict(d2=inner("d2", torch.float32) if "d2" in outputs else None, idx=inner("idx", torch.int32) if "idx" in outputs else None,
                words=inner("table", torch.int64) if "table" in outputs else None, info=inner("info", torch.int64))


def compare(got, query, target, flow=None, radius=2.0, groups=None, G=1, edges=(), label=""):
    """the call's outputs against the restatement: d2 and idx bit for bit, the table's counts equal, each of its sums within
    (rows - 1) 2^-53 sum of math.fsum -- the bound of a fixed-order fp64 sum of `rows` non-negative terms, as
    tests/test_gpu_segments.py derives it --, the bad rows counted.  -> the restatement's (d2, idx, table, info)"""
    d2, idx, tab, info = rr.residual(query, target, flow, radius, groups, G, edges)
    if got["d2"] is not None:
        assert np.array_equal(got["d2"].view(np.int32), d2.view(np.int32)), (label, "d2", np.flatnonzero(got["d2"] != d2)[:8])
    if got["idx"] is not None:
        assert np.array_equal(got["idx"], idx), (label, "idx", np.flatnonzero(got["idx"] != idx)[:8])
    assert (int(got["info"][0]), int(got["info"][1])) == (info["bad_queries"], info["bad_targets"]), label
    if got["words"] is not None:
        E = len(edges)
        w = got["words"].reshape(G, E + 4)
        assert np.array_equal(w[:, 0], tab["rows"]) and np.array_equal(w[:, 1], tab["hits"]), label
        assert np.array_equal(w[:, 2:2 + E], tab["under"]), label
        for col, key in ((2 + E, "dsum"), (3 + E, "ddsum")):
            sums = np.ascontiguousarray(w[:, col]).view(np.float64)
            bound = np.maximum(tab["rows"] - 1, 0) * 2.0 ** -53 * tab[key]
            assert (np.abs(sums - tab[key]) <= bound).all(), (label, key, sums, tab[key], bound)
    return d2, idx, tab, info


def check(query, target, flow=None, radius=2.0, groups=None, G=1, edges=(), label="", **kw):
    got = run(query, target, flow, radius, groups, G, edges, **kw)
    want = compare(got, query, target, flow, radius, groups, G, edges, label)
    return got, want


def scene(n, m, seed, span=6.0, radius=1.0, centre=(0.0, 0.0, 0.0), G=1, bad=False):
    """m targets uniform in a cube of edge 2 * span around `centre`; the queries: a third next to a target (inside the radius),
    a third anywhere in the cube, a third up to two radii outside it; a flow of up to half a radius.  bad: a few NaN, Inf, pad
    and out-of-range rows in both clouds and a few groups outside [0, G).  -> (query, target, flow, groups)"""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    t = rng.uniform(-span, span, (m, 3)) + c
    q = rng.uniform(-span - 2 * radius, span + 2 * radius, (n, 3)) + c
    if m:
        near = rng.random(n) < 1 / 3
        q[near] = t[rng.integers(0, m, int(near.sum()))] + rng.normal(0.0, radius / 3, (int(near.sum()), 3))
    f = rng.uniform(-radius / 2, radius / 2, (n, 3))
    q = q - f
    g = rng.integers(0, G, n).astype(np.int32)
    q, t, f = q.astype(np.float32), t.astype(np.float32), f.astype(np.float32)
    if bad:
        specials = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e8, 1e8, 1e8], [1.5e6, 0, 0], [0, -1000001.0, 0]], np.float32)
        for arr in (q, t):
            k = min(len(arr), 2 * len(specials))
            if k:
                arr[rng.choice(len(arr), k, replace=False)] = specials[rng.integers(0, len(specials), k)]
        if n >= 8:
            f[rng.choice(n, 2, replace=False)] = np.array([np.nan, 0, 0], np.float32)
            g[rng.choice(n, 3, replace=False)] = np.array([-1, G, G + 7], np.int32)
    return q, t, f, g

"""What the GPU tests of icpflow_nn_residual_segments share, in the style of tests/residual_device.py: one call on buffers the
test owns -- every output between two guards in its own allocation, poisoned beforehand, the workspace of EXACTLY the size the
library asks for, filled with 0xFF and guarded too -- and the comparison with tests/segment_residual_restatement.py.  Not a
test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd                  # noqa: E402
import segment_residual_restatement as sr     # noqa: E402
import table_restatement as tr                # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
OUTPUTS = ("d2_before", "d2_after")           # the optional ones
COLS = 18


def run(before, after, flow, labels, target, radius=2.0, edges=(), Lmax=4096, outputs=OUTPUTS, same_after=False, poison=0xA5,
        ws_poison=0xFF, shift=0, short=0, expect=0, expect_message=None):
    """One call on the current stream.  same_after: d_after is the very pointer of d_before (`after` is not read).  expect 0:
    status 0 asserted, every guard intact, an optional output not asked for untouched, the table's rows from *d_num on (all
    of them when it is negative) still poison -> dict(num int, table float64 [num, 18], d2_before, d2_after float32 [n] or None,
    info int64 [6]).  expect != 0: that status (and `expect_message` in the message) asserted, every byte of every buffer as it
    was.  shift: the workspace that many bytes further on; short: that many bytes fewer than the library asks for."""
    from icp_flow_amd import _lib
    L, p = _lib._L, _lib.ptr
    b = upload(np.asarray(before, np.float32).reshape(-1, 3), np.float32)
    a = b if same_after else upload(np.asarray(after, np.float32).reshape(-1, 3), np.float32)
    t = upload(np.asarray(target, np.float32).reshape(-1, 3), np.float32)
    f = None if flow is None else upload(np.asarray(flow, np.float32).reshape(-1, 3), np.float32)
    lab = upload(np.asarray(labels, np.float32).reshape(-1), np.float32)
    n, m, E = b.shape[0], t.shape[0], len(edges)
    ed = np.ascontiguousarray(edges, dtype=np.float64)
    need = int(L.icpflow_nn_residual_segments_workspace_bytes(n, m, Lmax, E))
    sizes = dict(d2_before=4 * n, d2_after=4 * n, table=8 * COLS * max(Lmax, 0), num=4, info=48, ws=max(need, 16) + shift)
    bufs = {k: rd._guarded(v, ws_poison if k == "ws" else poison) for k, v in sizes.items()}
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].data_ptr() + GUARD + off)   # noqa: E731
    held = {k: v.clone() for k, v in bufs.items()}
    rc = L.icpflow_nn_residual_segments(p(b), p(a), p(f), p(lab), n, p(t), m, float(radius), ed.ctypes.data_as(ctypes.c_void_p) if E else None, E,
                                        at("table"), Lmax, at("num"), at("d2_before") if "d2_before" in outputs else None,
                                        at("d2_after") if "d2_after" in outputs else None, at("info"), at("ws", shift),
                                        ctypes.c_size_t(need - short), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == expect, (rc, msg)
    if expect != 0:
        assert expect_message is None or expect_message in msg, msg
        assert all(torch.equal(bufs[k], held[k]) for k in bufs), "a refused call wrote something"
        return None
    for k, v in bufs.items():
        assert rd._guards_intact(v, sizes[k]), f"guard of {k} changed"
    for k in OUTPUTS:
        if k not in outputs:
            assert torch.equal(bufs[k], held[k]), k
    inner = lambda k, dt: bufs[k][GUARD: GUARD + sizes[k]].clone().view(dt).cpu().numpy()   # noqa: E731
    num = int(inner("num", torch.int32)[0])
    written = max(num, 0) * COLS * 8
    assert torch.equal(bufs["table"][GUARD + written:], held["table"][GUARD + written:]), "rows from *d_num on were written"
    return dict(num=num, table=inner("table", torch.float64)[: max(num, 0) * COLS].reshape(-1, COLS),
                d2_before=inner("d2_before", torch.float32) if "d2_before" in outputs else None,
                d2_after=inner("d2_after", torch.float32) if "d2_after" in outputs else None, info=inner("info", torch.int64))


def compare(got, want, edges, label=""):
    """the call's outputs against the restatement (sr.residual's dict): the labels bit for bit (as float32), rows and every
    count equal, each sum within (rows - 1) 2^-53 sum of math.fsum -- the bound of a fixed-order fp64 sum of `rows`
    non-negative terms, the one tests/residual_device.py uses --, the per-row d2 bit for bit, the bad rows counted."""
    L, E = len(want["rows"]), len(edges)
    assert got["num"] == L, (label, got["num"], L)
    t = got["table"]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(t[:, 0].astype(np.float32).view(np.uint32), tr.quiet(want["label_bits"])), (label, "labels")
    assert np.array_equal(t[:, 1], want["rows"]), (label, "rows")
    for at, side in ((2, "before"), (2 + sr.SIDE, "after")):
        w = want[side]
        assert np.array_equal(t[:, at], w["rows"]) and np.array_equal(t[:, at + 1], w["hits"]), (label, side, "good rows / hits")
        assert np.array_equal(t[:, at + 2: at + 2 + E], w["under"]) and (t[:, at + 2 + E: at + 2 + sr.MAX_EDGES] == 0).all(), (label, side, "under")
        for col, key in ((at + 6, "dsum"), (at + 7, "ddsum")):
            bound = np.maximum(w["rows"] - 1, 0) * 2.0 ** -53 * w[key]
            assert (np.abs(t[:, col] - w[key]) <= bound).all(), (label, side, key, np.abs(t[:, col] - w[key]).max())
    for k in OUTPUTS:
        if got[k] is not None:
            assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (label, k)
    assert tuple(int(v) for v in got["info"][:3]) == want["info"] and int(got["info"][5]) == 0, (label, got["info"], want["info"])


def check(before, after, flow, labels, target, radius=2.0, edges=(), Lmax=4096, label="", **kw):
    got = run(before, after, flow, labels, target, radius, edges, Lmax, **kw)
    want = sr.residual(before, before if kw.get("same_after") else after, flow, labels, target, radius, edges)
    compare(got, want, edges, label)
    return got, want


def scene(sizes, m, seed, span=5.0, radius=1.0, labels=None, bad=False):
    """a cloud of segments of the given sizes, their rows shuffled over the cloud: `before` near m targets uniform in a cube (a
    third next to a target, the rest anywhere up to two radii outside), `after` = before + a jitter, and a flow of up to half a
    radius.  labels: one value per segment (default 0, 1, 2, ...).  -> (before, after, flow, labels float32 [n], target)"""
    q, t, f, _ = rd.scene(int(sum(sizes)), m, seed, span=span, radius=radius, bad=bad)
    rng = np.random.default_rng(seed + 1)
    values = np.arange(len(sizes), dtype=np.float32) if labels is None else np.asarray(labels, np.float32)
    lab = np.repeat(values, sizes)[rng.permutation(len(q))]
    after = (q + rng.normal(0.0, radius / 10, q.shape)).astype(np.float32)
    return q, after, f, lab, t

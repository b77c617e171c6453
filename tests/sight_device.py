"""What the GPU tests of icpflow_sight_build / _query / _segments share, in the style of tests/segment_residual_device.py: one
call on buffers the test owns -- every output between two guards in its own allocation, poisoned beforehand, the workspace of
EXACTLY the size the library asks for, filled with 0xFF and guarded too -- and the comparison, array_equal throughout, with
tests/sight_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd                  # noqa: E402
import sight_restatement as S                 # noqa: E402
import table_restatement as tr                # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
COLS = 24
F = np.float32


def _args(view_params, origin):
    from icp_flow_amd import _lib
    p = _lib.SightParams.defaults(**view_params)
    o = np.ascontiguousarray(origin, dtype=np.float64)
    return p, o, ctypes.byref(p), o.ctypes.data_as(ctypes.c_void_p)


def _call(fn, sizes, poisons, call, expect, expect_message):
    """the guarded buffers of one call: -> (bufs, inner) after the asserts every call shares"""
    from icp_flow_amd import _lib
    bufs = {k: rd._guarded(v, poisons.get(k, 0xA5)) for k, v in sizes.items()}
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].data_ptr() + GUARD + off)   # noqa: E731
    held = {k: v.clone() for k, v in bufs.items()}
    rc = call(at)
    msg = _lib._L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == expect, (fn, rc, msg)
    if expect != 0:
        assert expect_message is None or expect_message in msg, msg
        assert all(torch.equal(bufs[k], held[k]) for k in bufs), "a refused call wrote something"
        return None, None, held
    for k, v in bufs.items():
        assert rd._guards_intact(v, sizes[k]), f"{fn}: guard of {k} changed"
    inner = lambda k, dt: bufs[k][GUARD: GUARD + sizes[k]].clone().view(dt).cpu().numpy()   # noqa: E731
    return bufs, inner, held


def build(target, origin=(0, 0, 0), poison=0xA5, expect=0, expect_message=None, **view_params):
    """icpflow_sight_build on the current stream.  -> dict(image uint32 [2, H, W], info int64 [3])"""
    from icp_flow_amd import _lib
    p, o, pp, po = _args(view_params, origin)
    t = upload(np.asarray(target, F).reshape(-1, 3), F)
    sizes = dict(image=8 * p.W * p.H, info=24)
    bufs, inner, _ = _call("build", sizes, dict(image=poison, info=poison),
                           lambda at: _lib._L.icpflow_sight_build(_lib.ptr(t), t.shape[0], po, pp, at("image"), at("info"), _lib.stream(DEV)),
                           expect, expect_message)
    if bufs is None:
        return None
    return dict(image=inner("image", torch.int32).view(np.uint32).reshape(2, p.H, p.W), info=inner("info", torch.int64))


def query(image, points, flow=None, origin=(0, 0, 0), near=True, poison=0xA5, expect=0, expect_message=None, **view_params):
    """icpflow_sight_query against a host image (uploaded).  -> dict(code int32 [n], near float32 [n] or None, counts int64 [6])"""
    from icp_flow_amd import _lib
    p, o, pp, po = _args(view_params, origin)
    img = upload(np.ascontiguousarray(image).view(np.int32), np.int32)
    q = upload(np.asarray(points, F).reshape(-1, 3), F)
    f = None if flow is None else upload(np.asarray(flow, F).reshape(-1, 3), F)
    n = q.shape[0]
    sizes = dict(code=4 * n, near=4 * n, counts=48)
    bufs, inner, held = _call("query", sizes, dict(code=poison, near=poison, counts=poison),
                              lambda at: _lib._L.icpflow_sight_query(_lib.ptr(img), pp, po, _lib.ptr(q), _lib.ptr(f), n, at("code"), at("near") if near else None,
                                                                     at("counts"), _lib.stream(DEV)), expect, expect_message)
    if bufs is None:
        return None
    if not near:
        assert torch.equal(bufs["near"], held["near"]), "near"
    return dict(code=inner("code", torch.int32), near=inner("near", torch.float32) if near else None, counts=inner("counts", torch.int64))


def check_frame(target, points, flow=None, origin=(0, 0, 0), label="", **view_params):
    """build and query against the restatement, bit for bit.  -> (image dict, query dict, the restatement's (image, code))"""
    v = S.view(origin, **view_params)
    want_image, want_info = S.build(v, target)
    got = build(target, origin, **view_params)
    assert np.array_equal(got["image"], want_image), (label, "image", np.argwhere(got["image"] != want_image)[:8])
    assert tuple(int(x) for x in got["info"]) == want_info, (label, got["info"], want_info)
    code, near, counts = S.query(v, want_image, points, flow)
    seen = query(got["image"], points, flow, origin, **view_params)
    assert np.array_equal(seen["code"], code), (label, "code", np.flatnonzero(seen["code"] != code)[:8])
    assert np.array_equal(seen["near"].view(np.uint32), near.view(np.uint32)), (label, "near")
    assert seen["counts"].tolist() == counts, (label, seen["counts"], counts)
    return got, seen, (want_image, code)


OUTPUTS = ("code_before", "code_after")       # the optional outputs
INPUTS = ("d2_before", "d2_after", "flow")    # the optional inputs


def segments(image, before, after, flow, labels, d2_before=None, d2_after=None, far=0.1, Lmax=4096, origin=(0, 0, 0), outputs=OUTPUTS,
             same_after=False, poison=0xA5, ws_poison=0xFF, shift=0, short=0, expect=0, expect_message=None, **view_params):
    """icpflow_sight_segments on the current stream, against a host image.  expect 0: status 0 asserted, every guard intact, an
    optional output not asked for untouched, the table's rows from *d_num on (all of them when it is negative) still poison
    -> dict(num, table float64 [num, 24], code_before, code_after int32 [n] or None, info int64 [12]).  expect != 0: that
    status asserted, every byte of every buffer as it was."""
    from icp_flow_amd import _lib
    L, ptr = _lib._L, _lib.ptr
    p, o, pp, po = _args(view_params, origin)
    img = upload(np.ascontiguousarray(image).view(np.int32), np.int32)
    b = upload(np.asarray(before, F).reshape(-1, 3), F)
    a = b if same_after else upload(np.asarray(after, F).reshape(-1, 3), F)
    f = None if flow is None else upload(np.asarray(flow, F).reshape(-1, 3), F)
    lab = upload(np.asarray(labels, F).reshape(-1), F)
    d2b, d2a = (None if d is None else upload(np.asarray(d, F).reshape(-1), F) for d in (d2_before, d2_after))
    n = b.shape[0]
    need = int(L.icpflow_sight_segments_workspace_bytes(n, Lmax))
    sizes = dict(code_before=4 * n, code_after=4 * n, table=8 * COLS * max(Lmax, 0), num=4, info=96, ws=max(need, 16) + shift)
    bufs, inner, held = _call("segments", sizes, dict(ws=ws_poison, code_before=poison, code_after=poison, table=poison, num=poison, info=poison),
                              lambda at: L.icpflow_sight_segments(ptr(img), pp, po, ptr(b), ptr(a), ptr(f), ptr(lab), n, ptr(d2b), ptr(d2a), float(far),
                                                                  at("table"), Lmax, at("num"), at("code_before") if "code_before" in outputs else None,
                                                                  at("code_after") if "code_after" in outputs else None, at("info"), at("ws", shift),
                                                                  ctypes.c_size_t(need - short), _lib.stream(DEV)), expect, expect_message)
    if bufs is None:
        return None
    for k in OUTPUTS:
        if k not in outputs:
            assert torch.equal(bufs[k], held[k]), k
    num = int(inner("num", torch.int32)[0])
    written = max(num, 0) * COLS * 8
    assert torch.equal(bufs["table"][GUARD + written:], held["table"][GUARD + written:]), "rows from *d_num on were written"
    return dict(num=num, table=inner("table", torch.float64)[: max(num, 0) * COLS].reshape(-1, COLS),
                code_before=inner("code_before", torch.int32) if "code_before" in outputs else None,
                code_after=inner("code_after", torch.int32) if "code_after" in outputs else None, info=inner("info", torch.int64))


def compare_segments(got, want, label=""):
    """the call's outputs against S.segments' dict: the labels bit for bit (as float32), every count equal, the per-row codes
    equal, the twelve counts equal"""
    assert got["num"] == len(want["rows"]), (label, got["num"], len(want["rows"]))
    t = got["table"]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(t[:, 0].astype(F).view(np.uint32), tr.quiet(want["label_bits"])), (label, "labels")
    assert np.array_equal(t[:, 1:], want["table"][:, 1:]), (label, "table", np.argwhere(t[:, 1:] != want["table"][:, 1:])[:8])
    for k in OUTPUTS:
        if got[k] is not None:
            assert np.array_equal(got[k], want[k]), (label, k)
    assert got["info"].tolist() == want["info"], (label, got["info"], want["info"])


def check_segments(target, before, after, flow, labels, d2_before=None, d2_after=None, far=0.1, Lmax=4096, origin=(0, 0, 0), label="",
                   same_after=False, outputs=OUTPUTS, **kw):
    """the image by the restatement (build has its own tests), the segments' call against S.segments"""
    view_params = {k: kw[k] for k in kw if k in S.START}
    v = S.view(origin, **view_params)
    image, _ = S.build(v, target)
    got = segments(image, before, after, flow, labels, d2_before, d2_after, far, Lmax, origin, outputs, same_after, **kw)
    want = S.segments(v, image, before, before if same_after else after, flow, labels, d2_before, d2_after, far)
    compare_segments(got, want, label)
    return got, want, image

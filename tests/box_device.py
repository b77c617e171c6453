"""What the GPU tests of icpflow_segment_boxes and icpflow_pair_objects share, in the manner of tests/match_eval_device.py: the
raw call on buffers the test owns -- a workspace of EXACTLY the size the library asks for, filled with 0xFF (NaN floats, -1
integers), between two guards, and every output between two guards in an allocation of its own, poisoned beforehand -- and the
comparison, np.array_equal throughout, with tests/box_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_restatement as br             # noqa: E402
import residual_device as rd             # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, OUT_POISON = 0xFF, 0xA5
POISON_WORD = np.uint64(0xA5A5A5A5A5A5A5A5)      # (as a float64 -1.9e-129: no result of these cases)


def cluster_table(points, labels, Lmax):
    """icpflow_cluster_table on the device -> (order int64 [n], table float64 [Lmax, 9], num int32 [1]) device tensors"""
    from icp_flow_amd import _lib
    p, lab = upload(np.asarray(points, F).reshape(-1, 3), F), upload(np.asarray(labels, F).reshape(-1), F)
    n = int(p.shape[0])
    order = torch.empty(n, dtype=torch.int64, device=DEV)
    table = torch.full((Lmax, 9), float("nan"), dtype=torch.float64, device=DEV)
    num = torch.empty(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(_lib._L.icpflow_cluster_table_workspace_bytes(n, Lmax)), dtype=torch.uint8, device=DEV)
    _lib.call("icpflow_cluster_table", _lib.ptr(p), _lib.ptr(lab), n, _lib.ptr(order), _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(ws),
              ctypes.c_size_t(ws.numel()), _lib.stream(DEV))
    torch.cuda.synchronize()
    return order, table, num


def run_boxes(points, order, table, num, dirs, delta, stream=None):
    """One call of icpflow_segment_boxes.  points: numpy [n, 3]; order, table, num: device tensors (a cluster table's, or
    hand-made).  Status 0, the guards of the workspace and of d_boxes intact, rows from *d_num on untouched, every word of the
    rows before it written.  -> (boxes float64 [L, 16] on the host, the bytes of the whole output buffer)"""
    from icp_flow_amd import _lib
    L, ptr = _lib._L, _lib.ptr
    p = upload(np.asarray(points, F).reshape(-1, 3), F)
    n, Lmax = int(p.shape[0]), int(table.shape[0])
    d = np.ascontiguousarray(dirs, F).reshape(-1, 2)
    need = int(L.icpflow_segment_boxes_workspace_bytes(n, Lmax, len(d)))
    assert need > 0 and need % 256 == 0
    ws = rd._guarded(need, WS_POISON)
    size = Lmax * br.BOX_COLS * 8
    out = rd._guarded(size, OUT_POISON)
    torch.cuda.synchronize()                                # (the uploads and the poison ran on the default stream)
    with torch.cuda.stream(stream):
        rc = L.icpflow_segment_boxes(ptr(p), n, ptr(order), ptr(table), ptr(num), Lmax, d.ctypes.data_as(ctypes.c_void_p), len(d), float(delta),
                                     ctypes.c_void_p(out.data_ptr() + GUARD), ctypes.c_void_p(ws.data_ptr() + GUARD), ctypes.c_size_t(need),
                                     _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    assert rd._guards_intact(out, size), "guard of d_boxes changed"
    raw = out[GUARD: GUARD + size].clone().cpu().numpy()
    words = raw.view(np.uint64).reshape(Lmax, br.BOX_COLS)
    written = br.segments_of(int(num.item()), Lmax)
    assert (words[written:] == POISON_WORD).all(), "d_boxes from *d_num on was written"
    assert not (words[:written] == POISON_WORD).any(), "words of d_boxes left unwritten"
    return raw.view(np.float64).reshape(Lmax, br.BOX_COLS)[:written].copy(), raw.tobytes()


def want_boxes(points, order, table, num, dirs, delta):
    return br.segment_boxes(points, order.cpu().numpy(), table.cpu().numpy(), int(num.item()), dirs, delta, Lmax=int(table.shape[0]))


def same(got, want, label=""):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    equal = (got == want) | (np.isnan(got) & np.isnan(want))
    assert equal.all(), (label, np.argwhere(~equal)[:8].tolist(), got[~equal][:8], want[~equal][:8])


def check_boxes(points, labels=None, dirs=None, delta=0.1, Lmax=64, table=None, label="", stream=None):
    """the call against the restatement on the same cluster table -> (boxes, bytes)"""
    dirs = br.directions(90) if dirs is None else dirs
    order, ctable, num = cluster_table(points, labels, Lmax) if table is None else table
    got, raw = run_boxes(points, order, ctable, num, dirs, delta, stream)
    same(got, want_boxes(points, order, ctable, num, dirs, delta), label)
    return got, raw


def run_objects(boxes_src, num_src, boxes_dst, num_dst, pairs, T, seconds=0.1, min_speed=0.5):
    """One call of icpflow_pair_objects on numpy inputs (boxes_dst None: no destination table).  -> (objects [P, 24], counts [4]);
    the guards intact, every word of the P rows and the four counts written."""
    from icp_flow_amd import _lib
    L, ptr = _lib._L, _lib.ptr
    bs = np.asarray(boxes_src, np.float64).reshape(-1, br.BOX_COLS)
    Lmax = max(len(bs), 1 if boxes_dst is None else len(boxes_dst), 1)

    def table(b):
        t = np.full((Lmax, br.BOX_COLS), np.nan)
        t[:len(b)] = b
        return upload(t, np.float64)

    d_bs, d_ns = table(bs), upload(np.array([num_src]), np.int32)
    d_bd = d_nd = None
    if boxes_dst is not None:
        d_bd, d_nd = table(np.asarray(boxes_dst, np.float64).reshape(-1, br.BOX_COLS)), upload(np.array([num_dst]), np.int32)
    pairs = np.asarray(pairs, F)
    P = len(pairs)
    stride = int(pairs.shape[1]) if P else 2
    d_pairs = upload(pairs, F) if P else None
    d_T = upload(np.asarray(T, F).reshape(P, 16), F) if P else None
    params = _lib.ObjectParams.defaults(seconds=seconds, min_speed=min_speed)
    sizes = dict(objects=P * br.OBJECT_COLS * 8, counts=32)
    bufs = {k: rd._guarded(v, OUT_POISON) for k, v in sizes.items()}
    at = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + GUARD)   # noqa: E731
    torch.cuda.synchronize()
    rc = L.icpflow_pair_objects(ptr(d_bs), ptr(d_ns), ptr(d_bd), ptr(d_nd), Lmax, ptr(d_pairs), P, stride, ptr(d_T), ctypes.byref(params),
                                at("objects"), at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    for k, b in bufs.items():
        assert rd._guards_intact(b, sizes[k]), f"guard of {k} changed"
    inner = lambda k: bufs[k][GUARD: GUARD + sizes[k]].clone().cpu().numpy()   # noqa: E731
    words = inner("objects").view(np.uint64)
    assert not (words == POISON_WORD).any(), "words of d_objects left unwritten"
    return words.view(np.float64).reshape(P, br.OBJECT_COLS).copy(), inner("counts").view(np.int64).copy()


def check_objects(boxes_src, num_src, boxes_dst, num_dst, pairs, T, seconds=0.1, min_speed=0.5, label=""):
    got, counts = run_objects(boxes_src, num_src, boxes_dst, num_dst, pairs, T, seconds, min_speed)
    Lmax = max(len(boxes_src), 1 if boxes_dst is None else len(boxes_dst), 1)
    want, want_counts = br.pair_objects(boxes_src, num_src, boxes_dst, num_dst, np.asarray(pairs, F).reshape(len(got), -1) if len(got) else np.zeros((0, 2), F),
                                        np.asarray(T, F).reshape(len(got), 16), seconds, min_speed, Lmax=Lmax)
    same(got, want, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return got, counts

"""What the GPU tests of icpflow_rows_carry, icpflow_pair_row_ids, icpflow_object_tracks_extend_side and
icpflow_object_tracks_path share, in the manner of tests/track_device.py: the raw call on buffers the test owns -- a workspace
of EXACTLY the size the library asks for, filled with 0xFF, between two guards, and every output between two guards in an
allocation of its own, poisoned beforehand -- and the comparison, np.array_equal (NaN = NaN, the bits of d2) throughout, with
tests/carry_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carry_restatement as cr           # noqa: E402
import residual_device as rd             # noqa: E402
import track_device as td                # noqa: E402
import track_restatement as trk          # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, POISON_WORD = td.WS_POISON, td.POISON_WORD
Buffers, same = td.Buffers, td.same


def _ws(need):
    assert need > 0 and need % 256 == 0
    return rd._guarded(need, WS_POISON)


def run_carry(prev, prev_id, pose, nxt, radius=cr.CARRY_RADIUS, min_share=cr.CARRY_MIN_SHARE, per_row=True, stream=None):
    """One call of icpflow_rows_carry on numpy inputs -> dict as carry_restatement.rows_carry's (d2, idx None without per_row),
    plus `raw`"""
    from icp_flow_amd import _lib
    L = _lib._L
    prev, nxt = np.asarray(prev, F).reshape(-1, 3), np.asarray(nxt, F).reshape(-1, 3)
    prev_id = np.asarray(prev_id, np.int32).reshape(-1)
    m, n = len(prev), len(nxt)
    d_prev, d_pid, d_next = (upload(prev, F) if m else None), (upload(prev_id, np.int32) if m else None), (upload(nxt, F) if n else None)
    h_pose = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(16))
    need = int(L.icpflow_rows_carry_workspace_bytes(n, m))
    ws = _ws(need)
    out = Buffers(id=4 * n, d2=4 * n, idx=4 * n, counts=8 * cr.CARRY_COUNTS)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_rows_carry(_lib.ptr(d_prev), _lib.ptr(d_pid), m, h_pose.ctypes.data_as(ctypes.c_void_p), _lib.ptr(d_next), n, float(radius),
                                  float(min_share), out.at("id") if n else None, out.at("d2") if per_row else None, out.at("idx") if per_row else None,
                                  out.at("counts"), ctypes.c_void_p(ws.data_ptr() + GUARD), ctypes.c_size_t(need), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out.check()
    if not per_row:
        assert (out.raw("d2") == td.OUT_POISON).all() and (out.raw("idx") == td.OUT_POISON).all(), "an output not asked for was written"
    return dict(id=out.raw("id").view(np.int32).copy(), d2=out.raw("d2").view(F).copy() if per_row else None,
                idx=out.raw("idx").view(np.int32).copy() if per_row else None, counts=out.raw("counts").view(np.int64).copy(),
                raw=b"".join(out.raw(k).tobytes() for k in sorted(out.sizes)))


def check_carry(prev, prev_id, pose, nxt, radius=cr.CARRY_RADIUS, min_share=cr.CARRY_MIN_SHARE, label="", want=None, **kw):
    got = run_carry(prev, prev_id, pose, nxt, radius, min_share, **kw)
    want = cr.rows_carry(prev, prev_id, pose, nxt, radius, min_share) if want is None else want
    assert np.array_equal(got["counts"], want["counts"]), (label, got["counts"], want["counts"])
    assert np.array_equal(got["id"], want["id"]), (label, "id", np.flatnonzero(got["id"] != want["id"])[:8])
    if got["idx"] is not None:
        assert np.array_equal(got["idx"], want["idx"]), (label, "idx", np.flatnonzero(got["idx"] != want["idx"])[:8])
        assert np.array_equal(got["d2"].view(np.int32), want["d2"].view(np.int32)), (label, "d2", np.flatnonzero(got["d2"] != want["d2"])[:8])
    return got, want


def run_row_ids(labels, pair_rows, col, pair_id, weight=None, weight_stride=1, stream=None):
    """One call of icpflow_pair_row_ids -> (ids int32 [n], counts int64 [3], the outputs' bytes).  weight: float64 [P] (spread
    `weight_stride` doubles apart on the device, NaN in between)"""
    from icp_flow_amd import _lib
    L = _lib._L
    labels = np.asarray(labels, F).reshape(-1)
    pair_id = np.asarray(pair_id, np.int32).reshape(-1)
    n, P = len(labels), len(pair_id)
    pairs = np.asarray(pair_rows, F).reshape(P, -1) if P else np.zeros((0, 2), F)
    stride = pairs.shape[1]
    d_labels, d_pairs, d_pid = (upload(labels, F) if n else None), (upload(pairs, F) if P else None), (upload(pair_id, np.int32) if P else None)
    d_w = None
    if weight is not None and P:
        spread = np.full((P, weight_stride), np.nan)
        spread[:, 0] = np.asarray(weight, np.float64).reshape(P)
        d_w = upload(spread, np.float64)
    need = int(L.icpflow_pair_row_ids_workspace_bytes(P))
    ws = _ws(need)
    out = Buffers(id=4 * n, counts=8 * cr.ROW_ID_COUNTS)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_pair_row_ids(_lib.ptr(d_labels), n, _lib.ptr(d_pairs), P, stride, int(col), _lib.ptr(d_pid), _lib.ptr(d_w), int(weight_stride),
                                    out.at("id") if n else None, out.at("counts"), ctypes.c_void_p(ws.data_ptr() + GUARD), ctypes.c_size_t(need),
                                    _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out.check()
    return out.raw("id").view(np.int32).copy(), out.raw("counts").view(np.int64).copy(), out.raw("id").tobytes() + out.raw("counts").tobytes()


def check_row_ids(labels, pair_rows, col, pair_id, weight=None, weight_stride=1, label="", stream=None):
    ids, counts, raw = run_row_ids(labels, pair_rows, col, pair_id, weight, weight_stride, stream)
    want, want_counts = cr.pair_row_ids(labels, pair_rows, col, pair_id, weight)
    assert np.array_equal(ids, want), (label, np.flatnonzero(ids != want)[:8], ids[:8], want[:8])
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return ids, counts, raw


def run_extend_side(labels, track_of_row, next_id, objects, side, gap, seconds, min_iou=0.5, Lmax=64, stream=None):
    """td.run_extend through icpflow_object_tracks_extend_side"""
    from icp_flow_amd import _lib
    L = _lib._L
    labels = np.asarray(labels, F).reshape(-1)
    n = len(labels)
    objects = np.zeros((0, 24)) if objects is None else np.asarray(objects, np.float64).reshape(-1, 24)
    P = len(objects)
    d_labels = upload(labels, F) if n else None
    d_objects = upload(objects, np.float64) if P else None
    need = int(L.icpflow_object_tracks_extend_workspace_bytes(n, Lmax))
    ws = _ws(need)
    out = Buffers(state=4 * n, next_id=4, segments=Lmax * trk.SEGMENT_COLS * 8, num=4, obs=P * trk.OBS_COLS * 8, counts=8 * trk.EXTEND_COUNTS)
    out.fill("state", np.asarray(track_of_row, np.int32).reshape(n))
    out.fill("next_id", np.array([next_id], np.int32))
    params = _lib.TrackParams.defaults(min_iou=min_iou)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_extend_side(_lib.ptr(d_labels), n, Lmax, out.at("state") if n else None, out.at("next_id"), _lib.ptr(d_objects), P,
                                                 int(side), int(gap), float(seconds), ctypes.byref(params), out.at("segments"), out.at("num"),
                                                 out.at("obs") if P else None, out.at("counts"), ctypes.c_void_p(ws.data_ptr() + GUARD),
                                                 ctypes.c_size_t(need), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out.check()
    num = int(out.raw("num").view(np.int32)[0])
    obs_words = out.raw("obs").view(np.uint64)
    assert not (obs_words == POISON_WORD).any(), "words of d_obs left unwritten"
    return dict(track_of_row=out.raw("state").view(np.int32).copy(), next_id=int(out.raw("next_id").view(np.int32)[0]),
                segments=td._rows(out.raw("segments"), trk.SEGMENT_COLS, max(num, 0), "d_segments"), num=num,
                obs=obs_words.view(np.float64).reshape(P, trk.OBS_COLS).copy(), counts=out.raw("counts").view(np.int64).copy(),
                raw=b"".join(out.raw(k).tobytes() for k in sorted(out.sizes)))


def check_extend_side(labels, track_of_row, next_id, objects, side, gap, seconds, min_iou=0.5, Lmax=64, label="", stream=None):
    got = run_extend_side(labels, track_of_row, next_id, objects, side, gap, seconds, min_iou, Lmax, stream)
    want = cr.extend_side(labels, track_of_row, next_id, objects, side, gap, seconds, min_iou, Lmax)
    assert (got["num"], got["next_id"]) == (want["num"], want["next_id"]), (label, got["num"], got["next_id"], want["num"], want["next_id"])
    assert np.array_equal(got["track_of_row"], want["track_of_row"]), (label, got["track_of_row"], want["track_of_row"])
    same(got["segments"], want["segments"], label + " segments")
    same(got["obs"], want["obs"], label + " obs")
    assert np.array_equal(got["counts"], want["counts"]), (label, got["counts"], want["counts"])
    return got


def run_path(obs, step, frames, T, max_dv=cr.MAX_DV, min_speed=cr.MIN_SPEED, stream=None):
    """One call of icpflow_object_tracks_path -> (paths [T, 24], counts [5], the outputs' bytes)"""
    from icp_flow_amd import _lib
    L = _lib._L
    obs = np.asarray(obs, np.float64).reshape(-1, trk.OBS_COLS)
    step = np.asarray(step, np.int32).reshape(-1)
    frames = np.asarray(frames, np.float64).reshape(-1, 12)
    M, Fn = len(obs), len(frames)
    assert len(step) == M
    d_obs, d_step, d_frames = (upload(obs, np.float64) if M else None), (upload(step, np.int32) if M else None), (upload(frames, np.float64) if Fn else None)
    out = Buffers(paths=T * cr.PATH_COLS * 8, counts=8 * cr.PATH_COUNTS)
    params = _lib.TrackPathParams.defaults(max_dv=max_dv, min_speed=min_speed)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_path(_lib.ptr(d_obs), _lib.ptr(d_step), M, _lib.ptr(d_frames), Fn, T, ctypes.byref(params),
                                          out.at("paths") if T else None, out.at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    paths = td._rows(out.raw("paths"), cr.PATH_COLS, T, "d_paths")
    return paths, out.raw("counts").view(np.int64).copy(), out.raw("paths").tobytes() + out.raw("counts").tobytes()


def check_path(obs, step, frames, T, max_dv=cr.MAX_DV, min_speed=cr.MIN_SPEED, label="", stream=None):
    paths, counts, raw = run_path(obs, step, frames, T, max_dv, min_speed, stream)
    want, want_counts = cr.path(obs, step, frames, T, max_dv, min_speed)
    same(paths, want, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return paths, counts, raw

"""What the GPU tests of icpflow_label_overlap, icpflow_object_tracks_extend and icpflow_object_tracks_fit share, in the manner
of tests/box_device.py: the raw call on buffers the test owns -- a workspace of EXACTLY the size the library asks for, filled
with 0xFF, between two guards, and every output between two guards in an allocation of its own, poisoned beforehand -- and the
comparison, np.array_equal (NaN = NaN) throughout, with tests/track_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_device as bd                  # noqa: E402
import residual_device as rd             # noqa: E402
import track_restatement as trk          # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, OUT_POISON, POISON_WORD = bd.WS_POISON, bd.OUT_POISON, bd.POISON_WORD
same = bd.same


class Buffers:
    """named output buffers, each poisoned between two guards"""

    def __init__(self, **sizes):
        self.sizes = sizes
        self.bufs = {k: rd._guarded(v, OUT_POISON) for k, v in sizes.items()}

    def at(self, k):
        return ctypes.c_void_p(self.bufs[k].data_ptr() + GUARD)

    def check(self):
        for k, b in self.bufs.items():
            assert rd._guards_intact(b, self.sizes[k]), f"guard of {k} changed"

    def raw(self, k):
        return self.bufs[k][GUARD: GUARD + self.sizes[k]].clone().cpu().numpy()

    def fill(self, k, array):
        a = np.ascontiguousarray(array)
        assert a.nbytes == self.sizes[k]
        self.bufs[k][GUARD: GUARD + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1)).to(DEV)


def _rows(raw, cols, written, name):
    """float64 [written, cols] of a table's bytes: every word of the rows before `written` written, none behind"""
    words = raw.view(np.uint64).reshape(-1, cols)
    assert (words[written:] == POISON_WORD).all(), f"{name} from its number on was written"
    assert not (words[:written] == POISON_WORD).any(), f"words of {name} left unwritten"
    return words[:written].view(np.float64).copy()


def run_overlap(a, b, Lmax=64, stream=None):
    """One call of icpflow_label_overlap -> (table_a, table_b, num_a, num_b, counts, the bytes of every output)"""
    from icp_flow_amd import _lib
    L = _lib._L
    a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
    n = len(a)
    da, db = (upload(a, F), upload(b, F)) if n else (None, None)
    need = int(L.icpflow_label_overlap_workspace_bytes(n, Lmax))
    assert need > 0 and need % 256 == 0
    ws = rd._guarded(need, WS_POISON)
    out = Buffers(table_a=Lmax * trk.OVERLAP_COLS * 8, table_b=Lmax * trk.OVERLAP_COLS * 8, num_a=4, num_b=4, counts=8 * trk.OVERLAP_COUNTS)
    torch.cuda.synchronize()                                # (the uploads and the poison ran on the default stream)
    with torch.cuda.stream(stream):
        rc = L.icpflow_label_overlap(_lib.ptr(da), _lib.ptr(db), n, Lmax, out.at("table_a"), out.at("num_a"), out.at("table_b"), out.at("num_b"),
                                     out.at("counts"), ctypes.c_void_p(ws.data_ptr() + GUARD), ctypes.c_size_t(need), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    out.check()
    num_a, num_b = int(out.raw("num_a").view(np.int32)[0]), int(out.raw("num_b").view(np.int32)[0])
    usable = num_a > 0 and num_b > 0
    ta = _rows(out.raw("table_a"), trk.OVERLAP_COLS, num_a if usable else 0, "d_table_a")
    tb = _rows(out.raw("table_b"), trk.OVERLAP_COLS, num_b if usable else 0, "d_table_b")
    counts = out.raw("counts").view(np.int64).copy()
    return ta, tb, num_a, num_b, counts, b"".join(out.raw(k).tobytes() for k in sorted(out.sizes))


def check_overlap(a, b, Lmax=64, label="", stream=None):
    ta, tb, num_a, num_b, counts, raw = run_overlap(a, b, Lmax, stream)
    wa, wb, wnum_a, wnum_b, wcounts = trk.label_overlap(a, b, Lmax)
    assert (num_a, num_b) == (wnum_a, wnum_b), (label, num_a, num_b, wnum_a, wnum_b)
    same(ta, wa, label + " A")
    same(tb, wb, label + " B")
    assert np.array_equal(counts, wcounts), (label, counts, wcounts)
    return ta, tb, counts, raw


def run_extend(labels, track_of_row, next_id, objects, gap, seconds, min_iou=0.5, Lmax=64, stream=None):
    """One call of icpflow_object_tracks_extend on numpy inputs -> dict as track_restatement.extend's, plus `raw`"""
    from icp_flow_amd import _lib
    L = _lib._L
    labels = np.asarray(labels, F).reshape(-1)
    n = len(labels)
    objects = np.zeros((0, 24)) if objects is None else np.asarray(objects, np.float64).reshape(-1, 24)
    P = len(objects)
    d_labels = upload(labels, F) if n else None
    d_objects = upload(objects, np.float64) if P else None
    need = int(L.icpflow_object_tracks_extend_workspace_bytes(n, Lmax))
    assert need > 0 and need % 256 == 0
    ws = rd._guarded(need, WS_POISON)
    out = Buffers(state=4 * n, next_id=4, segments=Lmax * trk.SEGMENT_COLS * 8, num=4, obs=P * trk.OBS_COLS * 8, counts=8 * trk.EXTEND_COUNTS)
    out.fill("state", np.asarray(track_of_row, np.int32).reshape(n))
    out.fill("next_id", np.array([next_id], np.int32))
    params = _lib.TrackParams.defaults(min_iou=min_iou)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_extend(_lib.ptr(d_labels), n, Lmax, out.at("state") if n else None, out.at("next_id"), _lib.ptr(d_objects), P,
                                            int(gap), float(seconds), ctypes.byref(params), out.at("segments"), out.at("num"),
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
                segments=_rows(out.raw("segments"), trk.SEGMENT_COLS, max(num, 0), "d_segments"), num=num,
                obs=obs_words.view(np.float64).reshape(P, trk.OBS_COLS).copy(), counts=out.raw("counts").view(np.int64).copy(),
                raw=b"".join(out.raw(k).tobytes() for k in sorted(out.sizes)))


def check_extend(labels, track_of_row, next_id, objects, gap, seconds, min_iou=0.5, Lmax=64, label="", stream=None):
    got = run_extend(labels, track_of_row, next_id, objects, gap, seconds, min_iou, Lmax, stream)
    want = trk.extend(labels, track_of_row, next_id, objects, gap, seconds, min_iou, Lmax)
    assert (got["num"], got["next_id"]) == (want["num"], want["next_id"]), (label, got["num"], got["next_id"], want["num"], want["next_id"])
    assert np.array_equal(got["track_of_row"], want["track_of_row"]), (label, got["track_of_row"], want["track_of_row"])
    same(got["segments"], want["segments"], label + " segments")
    same(got["obs"], want["obs"], label + " obs")
    assert np.array_equal(got["counts"], want["counts"]), (label, got["counts"], want["counts"])
    return got


def run_fit(obs, T, max_residual=0.2, min_speed=0.5, stream=None):
    """One call of icpflow_object_tracks_fit -> (tracks [T, 16], counts [5], the outputs' bytes)"""
    from icp_flow_amd import _lib
    L = _lib._L
    obs = np.asarray(obs, np.float64).reshape(-1, trk.OBS_COLS)
    M = len(obs)
    d_obs = upload(obs, np.float64) if M else None
    out = Buffers(tracks=T * trk.TRACK_COLS * 8, counts=8 * trk.FIT_COUNTS)
    params = _lib.TrackParams.defaults(max_residual=max_residual, min_speed=min_speed)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_fit(_lib.ptr(d_obs), M, T, ctypes.byref(params), out.at("tracks") if T else None, out.at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    tracks = _rows(out.raw("tracks"), trk.TRACK_COLS, T, "d_tracks")
    return tracks, out.raw("counts").view(np.int64).copy(), out.raw("tracks").tobytes() + out.raw("counts").tobytes()


def check_fit(obs, T, max_residual=0.2, min_speed=0.5, label="", stream=None):
    tracks, counts, raw = run_fit(obs, T, max_residual, min_speed, stream)
    want, want_counts = trk.fit(obs, T, max_residual, min_speed)
    same(tracks, want, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return tracks, counts, raw

"""What the GPU tests of the track fill share, in the manner of tests/repair_device.py: the raw calls of
icpflow_object_tracks_missing and icpflow_pairs_fill_candidates on buffers the test owns -- every output between two guards in
an allocation of its own, poisoned beforehand -- and the comparison, np.array_equal (NaN = NaN) throughout, with
tests/fill_restatement.py.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_device as bd                  # noqa: E402
import fill_restatement as fr            # noqa: E402
import residual_device as rd             # noqa: E402
import track_device as td                # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
POISON_WORD = bd.POISON_WORD
same, Buffers = bd.same, td.Buffers


def run_missing(obs, T, segments, num, gaps, seconds, max_residual=0.2, stream=None):
    """One call of icpflow_object_tracks_missing -> (plan [G, Lmax, 14] with fill_restatement.POISON in the rows that were not
    written, written bool [G, Lmax], counts [G, 4], the outputs' bytes)"""
    from icp_flow_amd import _lib
    L = _lib._L
    obs = np.asarray(obs, np.float64).reshape(-1, fr.OBS_COLS)
    segments = np.ascontiguousarray(segments, np.float64)
    G, Lmax, M = segments.shape[0], segments.shape[1], len(obs)
    d_obs = upload(obs, np.float64) if M else None
    d_seg, d_num = upload(segments, np.float64), upload(np.asarray(num, np.int32).reshape(G), np.int32)
    h_gap, h_sec = np.array(gaps, np.int32).reshape(G), np.array(seconds, np.float64).reshape(G)      # (copies: they are overwritten below)
    out = Buffers(plan=G * Lmax * fr.MISSING_COLS * 8, counts=G * fr.MISSING_COUNTS * 8)
    params = _lib.TrackParams.defaults(max_residual=max_residual)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_missing(_lib.ptr(d_obs), M, int(T), _lib.ptr(d_seg), _lib.ptr(d_num), G, Lmax, h_gap.ctypes.data_as(ctypes.c_void_p),
                                             h_sec.ctypes.data_as(ctypes.c_void_p), ctypes.byref(params), out.at("plan"), out.at("counts"), _lib.stream(DEV))
        h_gap[:], h_sec[:] = -5, -1.0                        # the host arrays were copied before the call returned
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    words = out.raw("plan").view(np.uint64).reshape(G, Lmax, fr.MISSING_COLS)
    untouched = words == POISON_WORD
    written = ~untouched.any(axis=2)
    assert (untouched.all(axis=2) | written).all(), "a row of d_plan written in part"
    plan = words.view(np.float64).copy()
    plan[~written] = fr.POISON
    return plan, written, out.raw("counts").view(np.int64).reshape(G, fr.MISSING_COUNTS).copy(), out.raw("plan").tobytes() + out.raw("counts").tobytes()


def check_missing(obs, T, segments, num, gaps, seconds, max_residual=0.2, label="", stream=None):
    plan, written, counts, raw = run_missing(obs, T, segments, num, gaps, seconds, max_residual, stream)
    want, want_written, want_counts = fr.missing(obs, T, segments, num, gaps, seconds, max_residual)
    assert np.array_equal(written, want_written), (label, "the rows written")
    same(plan.reshape(-1, fr.MISSING_COLS), want.reshape(-1, fr.MISSING_COLS), label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return plan, counts, raw


def run_candidates(q, boxes, num, pairs, radius=fr.FILL_RADIUS, max_rows=10000, stream=None):
    """One call of icpflow_pairs_fill_candidates -> (choice [K, 8], counts [4], the outputs' bytes); pairs float32 [P, stride]"""
    from icp_flow_amd import _lib
    L = _lib._L
    q, boxes = np.asarray(q, np.float64).reshape(-1, 3), np.ascontiguousarray(boxes, np.float64).reshape(-1, fr.BOX_COLS)
    pairs = np.asarray(pairs, F)
    K, Lmax, P = len(q), len(boxes), len(pairs)
    stride = pairs.shape[1] if P else 10
    d_q = upload(q, np.float64) if K else None
    d_boxes, d_num = upload(boxes, np.float64), upload(np.array([num], np.int32), np.int32)
    d_pairs = upload(pairs, F) if P else None
    out = Buffers(choice=K * fr.CHOICE_COLS * 8, counts=8 * fr.FILL_COUNTS)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_pairs_fill_candidates(_lib.ptr(d_q), K, _lib.ptr(d_boxes), _lib.ptr(d_num), Lmax, _lib.ptr(d_pairs), P, stride, float(radius), int(max_rows),
                                             out.at("choice") if K else None, out.at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    choice = td._rows(out.raw("choice"), fr.CHOICE_COLS, K, "d_choice")
    return choice, out.raw("counts").view(np.int64).copy(), out.raw("choice").tobytes() + out.raw("counts").tobytes()


def check_candidates(q, boxes, num, pairs, radius=fr.FILL_RADIUS, max_rows=10000, label="", stream=None):
    choice, counts, raw = run_candidates(q, boxes, num, pairs, radius, max_rows, stream)
    pairs = np.asarray(pairs, F)
    want, want_counts = fr.candidates(q, boxes, num, pairs[:, 0] if len(pairs) else [], radius, max_rows)
    same(choice, want, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return choice, counts, raw

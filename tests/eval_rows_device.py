"""What the GPU tests of the evaluation's row rules share, in the style of tests/match_eval_device.py: the raw calls of
icpflow_seq_metrics and icpflow_seq_segment_table on buffers the test owns -- a workspace of EXACTLY the size the library asks for,
filled with 0xFF, between two guards, and every output between two guards in an allocation of its own, poisoned beforehand -- and
the comparison with tests/seqeval_restatement.py and tests/segment_restatement.py where a sum may be NaN or infinite.
Not a test module."""
import ctypes
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_rows_cases as ec          # noqa: E402
import residual_device as rd          # noqa: E402
import segment_restatement as sg      # noqa: E402
import seqeval_restatement as sr      # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
WS_POISON, OUT_POISON = 0xFF, 0xA5
POISON_WORD = np.array([0xA5A5A5A5A5A5A5A5], np.uint64).view(np.int64)[0]      # (as a double -2.9e-131, as a count negative: no result)
U = 2.0 ** -53
CROP_MODES = ("none", "xy", "xyz")


def thresholds(pts):
    """the crop bounds as numpy compares them with an array of this type (utils_eval._threshold_for): rounded to it"""
    dt = np.asarray(pts).dtype.type
    return tuple(float(dt(v)) if dt is np.float32 else float(v) for v in (ec.RANGE_X, ec.RANGE_Y, ec.Z_MIN))


def binary(labels):
    a = np.asarray(labels)
    return np.where(a == 0, 0, np.where(a == 1, 1, 2)).astype(np.int32)


def _at(buf):
    return ctypes.c_void_p(buf.data_ptr() + GUARD)


def _words(buf, nbytes, what):
    """the payload of a guarded output as int64 words: the guards intact, no word left as the poison"""
    assert rd._guards_intact(buf, nbytes), f"guard of {what} changed"
    w = buf[GUARD: GUARD + nbytes].clone().view(torch.int64).cpu().numpy()
    assert not (w == POISON_WORD).any(), f"{what}: words left unwritten"
    return w


def run_metrics(s, crop="xyz", stream=None, bounds=None):
    """One raw call of icpflow_seq_metrics on sample `s` (eval_rows_cases) -> SimpleNamespace(table int64 [F,6,6] with zeros where the
    sums go, esum float64 [F,6], kept0, outside, bytes).  Status 0, the guards intact, every word of the table and of d_info written."""
    from icp_flow_amd import _lib
    d, F, m = s.data, s.F, len(s.pred)
    rx, ry, zmin = thresholds(d["raw_points"]) if bounds is None else bounds
    dev = [upload(np.asarray(d["raw_points"], np.float64).reshape(m, 3), np.float64), upload(d["time_indice"], np.int32), upload(binary(d["sd_labels"]), np.int32),
           upload(binary(d["fb_labels"]), np.int32), upload(np.asarray(d["scene_flow"], np.float64).reshape(m, 3), np.float64),
           upload(np.asarray(s.pred, np.float32).reshape(m, 3), np.float32)]
    need = int(_lib._L.icpflow_seq_metrics_workspace_bytes(m, F))
    assert need > 0
    ws, table, info = rd._guarded(need, WS_POISON), rd._guarded(F * 36 * 8, OUT_POISON), rd._guarded(16, OUT_POISON)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    with torch.cuda.stream(st):
        _lib.call("icpflow_seq_metrics", *[_lib.ptr(t) if m else None for t in dev], m, F, CROP_MODES.index(crop), rx, ry, zmin, _at(table), _at(info),
                  _at(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    torch.cuda.synchronize()
    assert rd._guards_intact(ws, need), "guard of the workspace changed"
    w, i = _words(table, F * 36 * 8, "table"), _words(info, 16, "d_info")
    t = w.reshape(F, 6, 6).copy()
    esum = np.ascontiguousarray(t[:, :, 1]).view(np.float64).copy()
    t[:, :, 1] = 0
    return SimpleNamespace(table=t, esum=esum, kept0=int(i[0]), outside=int(i[1]), bytes=w.tobytes() + i.tobytes())


def keep_rows(d, crop, bounds=None):
    """the crop as numpy applies it, in the points' own type; "xy" is crop_data's x-y half (utils_eval.py:33)"""
    raw = np.asarray(d["raw_points"])
    rx, ry, zmin = (ec.RANGE_X, ec.RANGE_Y, ec.Z_MIN) if bounds is None else bounds
    with np.errstate(invalid="ignore"):
        if crop == "none":
            return np.ones(len(raw), bool)
        keep = (np.abs(raw[:, 0]) < rx) & (np.abs(raw[:, 1]) < ry)
        return keep if crop == "xy" else keep & (raw[:, 2] > zmin)


def restate_metrics(s, crop="xyz", bounds=None):
    """tests/seqeval_restatement.table_numpy on the rows the crop keeps -> (table, numpy's sums, kept0, outside, fsum [F,6] of the
    finite cells, n [F,6])"""
    d, F = s.data, s.F
    keep = keep_rows(d, crop, bounds)
    kept = {k: np.asarray(v)[keep] for k, v in d.items()}
    with np.errstate(all="ignore"):
        table, esum, kept0 = sr.table_numpy(ec.args_for(F, eval_ground=True), kept, np.asarray(s.pred)[keep])
        e, _ = sr.errors(kept["scene_flow"], np.asarray(s.pred)[keep])
    t, sd, fb = kept["time_indice"], kept["sd_labels"], kept["fb_labels"]
    masks = (np.ones(len(t), bool), sd == 0, (sd == 0) & (fb == 0), (sd == 0) & (fb == 1), sd == 1, (sd == 1) & (fb == 1))
    exact = np.zeros((F, 6))
    for j in range(1, F):
        for c, mask in enumerate(masks):
            v = e[(t == j) & mask]
            exact[j, c] = math.fsum(v) if np.isfinite(v).all() else np.nan
    tim = np.asarray(d["time_indice"])
    return table, esum, kept0, int(((tim < 0) | (tim >= F)).sum()), exact, table[:, :, 0]


def check_metrics(got, s, crop="xyz", bounds=None, label=""):
    """Counts, kept0 and outside equal.  The sum of e of a gap's cell: NaN or infinite exactly where numpy's sum is; bit for bit the
    exactly rounded sum (math.fsum) where the cell holds one row or the sample's values add exactly in any order; else within
    (n - 1) 2^-53 sum e of it.  Row 0: the counts are the gap rows' sums, the sum of e is the gap rows added in gap order, bit for
    bit.  -> the largest error / bound seen"""
    table, numpy_sum, kept0, outside, exact, n = restate_metrics(s, crop, bounds)
    assert np.array_equal(got.table, table), (label, np.argwhere(got.table != table)[:8])
    assert (got.kept0, got.outside) == (kept0, outside), (label, got.kept0, kept0, got.outside, outside)
    assert np.array_equal(got.table[0], got.table[1:].sum(axis=0)), label
    worst = 0.0
    for j in range(1, s.F):
        for c in range(6):
            g, w = got.esum[j, c], numpy_sum[j, c]
            if not np.isfinite(w):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (label, j, c, g, w)
                continue
            bound = max(n[j, c] - 1, 0) * U * exact[j, c]
            if s.exact or n[j, c] <= 1:
                assert g == exact[j, c], (label, j, c, g, exact[j, c])
            else:
                assert abs(g - exact[j, c]) <= bound, (label, j, c, g, exact[j, c], bound)
                if bound > 0:
                    worst = max(worst, abs(g - exact[j, c]) / bound)
    acc = np.zeros(6)
    for j in range(1, s.F):
        acc = acc + got.esum[j]
    assert np.array_equal(got.esum[0], acc, equal_nan=True), label
    return worst


def run_segments(pts, labels, pred, gt, z_min, Lmax=64, stream=None):
    """One raw call of icpflow_seq_segment_table -> (table [Lmax,16] float64, num, bytes): the workspace exact, poisoned and guarded,
    the table and *d_num guarded and poisoned; rows below num written in every word, rows from num on untouched."""
    from icp_flow_amd import _lib
    n = len(labels)
    dev = [upload(np.asarray(pts, np.float64).reshape(n, 3), np.float64), upload(labels, np.float32),
           upload(None if gt is None else np.asarray(gt).reshape(n, 3), np.float64), upload(None if pred is None else np.asarray(pred).reshape(n, 3), np.float32)]
    need = int(_lib._L.icpflow_seq_segment_table_workspace_bytes(n, Lmax))
    assert need > 0
    ws, table, num = rd._guarded(need, WS_POISON), rd._guarded(Lmax * 16 * 8, OUT_POISON), rd._guarded(8, OUT_POISON)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    with torch.cuda.stream(st):
        _lib.call("icpflow_seq_segment_table", _lib.ptr(dev[0]), _lib.ptr(dev[1]), n, _lib.ptr(dev[2]), _lib.ptr(dev[3]), float(z_min), _at(table),
                  Lmax, _at(num), _at(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    torch.cuda.synchronize()
    assert rd._guards_intact(ws, need) and rd._guards_intact(table, Lmax * 16 * 8) and rd._guards_intact(num, 8), "a guard changed"
    k = int(num[GUARD: GUARD + 4].clone().view(torch.int32).item())
    assert (num[GUARD + 4: GUARD + 8] == OUT_POISON).all()            # *d_num is one int32
    w = table[GUARD: GUARD + Lmax * 16 * 8].clone().view(torch.int64).cpu().numpy().reshape(Lmax, 16)
    rows = max(min(k, Lmax), 0)
    assert not (w[:rows] == POISON_WORD).any(), "table: words of a reported row left unwritten"
    assert (w[rows:] == POISON_WORD).all(), "table: a row from num on was written"
    return w.view(np.float64), k, w[:rows].tobytes()


def check_segments(got, num, pts, labels, pred, gt, z_min, label=""):
    """Rows, kept, the four counts and num equal; the sum of e and the six coordinate sums NaN or infinite where the exactly rounded
    sum is, else within (kept - 1) 2^-53 sum |term| of it (tests/segment_restatement.check_table's bound).  -> largest error / bound"""
    with np.errstate(all="ignore"):
        want, _, absx, absm = sg.table_numpy(pts, labels, pred, gt, None if z_min == -np.inf else z_min)
    assert num == len(want), (label, num, len(want))
    got = got[:num]
    exact_cols = [0, 1, 2, 4, 5, 6, 7, 14, 15]
    assert np.array_equal(got[:, exact_cols], want[:, exact_cols]), (label, np.argwhere(got[:, exact_cols] != want[:, exact_cols])[:8])
    n = np.maximum(want[:, 2] - 1.0, 0.0)
    worst = 0.0
    with np.errstate(invalid="ignore"):
        scale = np.concatenate([np.abs(want[:, 3:4]), absx, absm], axis=1)
    for k, col in enumerate([3, 8, 9, 10, 11, 12, 13]):
        for c in range(num):
            g, w = got[c, col], want[c, col]
            if not np.isfinite(w):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (label, c, col, g, w)
                continue
            bound = n[c] * U * scale[c, k]
            assert abs(g - w) <= bound, (label, c, col, g, w, bound)
            if bound > 0:
                worst = max(worst, abs(g - w) / bound)
    return worst

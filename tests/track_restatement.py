"""Plain numpy restatement of the object tracks (include/icpflow_hip.h, "8(k) object tracks": icpflow_label_overlap,
icpflow_object_tracks_extend, icpflow_object_tracks_fit; csrc/overlap.hip, csrc/tracks.hip), written from the header's text.
Integers by np.unique and counting, ties by the stated rule; the fit in float64, one Python float operation per operation the
header writes out, in its order.  Not a test module."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_restatement as br             # noqa: E402
import table_restatement as tr           # noqa: E402

F = np.float32
OVERLAP_COLS, OVERLAP_COUNTS = 10, 4
SEGMENT_COLS, OBS_COLS, TRACK_COLS = 6, 13, 16
EXTEND_COUNTS, FIT_COUNTS = 6, 5
MAX_ID = 1 << 24
MIN_IOU, MAX_RESIDUAL, MIN_SPEED = 0.5, 0.2, 0.5


def segments(labels):
    """-> (rows float64 [L, 2] = (label, count) ascending as the cluster table reports them, seg int64 [n] = the segment of
    every row)"""
    labels = np.asarray(labels, F).reshape(-1)
    _, rows, _ = tr.table(labels)
    k = tr.key(labels)
    seg = np.searchsorted(np.unique(k), k).astype(np.int64)
    return rows[:, :2], seg


def linkable(label):
    return not (label < 0.0)              # a NaN is no negative number


def _links(pairs, counts, La, Lb):
    """per segment c of the first side: partner, inter, second, linked rows -- from (c, e, rows) triples sorted by (c, e)"""
    out = np.zeros((La, 4), np.int64)
    out[:, 0] = -1
    for c in range(La):
        sel = pairs[:, 0] == c
        e, v = pairs[sel, 1], counts[sel]
        if len(v) == 0:
            continue
        best = int(np.argmax(v))          # (the first maximum: the lowest e)
        others = np.delete(v, best)
        out[c] = e[best], v[best], others.max() if len(others) else 0, v.sum()
    return out


def label_overlap(a, b, Lmax=4096):
    """-> (table_a [La, 10], table_b [Lb, 10], num_a, num_b, counts int64 [4]); the tables are empty when a side overflows"""
    a, b = np.asarray(a, F).reshape(-1), np.asarray(b, F).reshape(-1)
    assert len(a) == len(b)
    if len(a) == 0:
        return np.zeros((0, OVERLAP_COLS)), np.zeros((0, OVERLAP_COLS)), 0, 0, np.zeros(OVERLAP_COUNTS, np.int64)
    (ra, sa), (rb, sb) = segments(a), segments(b)
    La, Lb = len(ra), len(rb)
    num_a, num_b = (La if La <= Lmax else -La), (Lb if Lb <= Lmax else -Lb)
    if num_a < 0 or num_b < 0:
        return np.zeros((0, OVERLAP_COLS)), np.zeros((0, OVERLAP_COLS)), num_a, num_b, np.zeros(OVERLAP_COUNTS, np.int64)
    ok_a = np.array([linkable(x) for x in ra[:, 0]]), np.array([linkable(x) for x in rb[:, 0]])
    both = ok_a[0][sa] & ok_a[1][sb]
    code, cnt = np.unique(sa[both] * Lb + sb[both], return_counts=True)
    ab = np.stack([code // Lb, code % Lb], axis=1).reshape(-1, 2)
    link_a = _links(ab, cnt, La, Lb)
    by_b = np.lexsort((ab[:, 0], ab[:, 1]))
    link_b = _links(ab[by_b][:, ::-1], cnt[by_b], Lb, La)
    tables = []
    for rows, link, other_rows, other_link in ((ra, link_a, rb, link_b), (rb, link_b, ra, link_a)):
        t = np.zeros((len(rows), OVERLAP_COLS))
        for c in range(len(rows)):
            p, inter, second, linked = (int(v) for v in link[c])
            t[c, 0:4] = rows[c, 0], rows[c, 1], linked, p
            if p >= 0:
                prows = other_rows[p, 1]
                t[c, 4:9] = other_rows[p, 0], inter, second, prows, 1.0 if other_link[p, 0] == c else 0.0
                t[c, 9] = float(inter) / ((rows[c, 1] + prows) - float(inter))
        tables.append(t)
    counts = np.array([link_a[:, 3].sum(), tables[0][:, 8].sum(), (link_a[:, 0] >= 0).sum(), (link_b[:, 0] >= 0).sum()], np.int64)
    return tables[0], tables[1], num_a, num_b, counts


def track_labels(track_of_row):
    t = np.asarray(track_of_row, np.int32)
    return np.where(t < 0, F(-1.0), t.astype(F)).astype(F)


def find_segment(table, L, label):
    return br.find_segment(table, L, label)


def extend(labels, track_of_row, next_id, objects, gap, seconds, min_iou=MIN_IOU, Lmax=4096):
    """-> dict(track_of_row int32 [n], next_id, segments [L, 6], num, obs [P, 13], counts int64 [6])"""
    labels = np.asarray(labels, F).reshape(-1)
    state = np.asarray(track_of_row, np.int32).copy()
    objects = np.zeros((0, br.OBJECT_COLS)) if objects is None else np.asarray(objects, np.float64).reshape(-1, br.OBJECT_COLS)
    ta, _, num_a, num_b, _ = label_overlap(labels, track_labels(state), Lmax)
    L = len(ta)
    link = np.array([linkable(x) for x in ta[:, 0]], bool).reshape(L)
    inherit = link & (ta[:, 3] >= 0) & (ta[:, 8] != 0) & (ta[:, 9] >= min_iou) if L else link
    fresh = link & ~inherit
    overflow = num_a < 0 or num_b < 0 or next_id < 0 or next_id > MAX_ID - int(fresh.sum())
    counts = np.zeros(EXTEND_COUNTS, np.int64)
    seg_id = np.full(L, -1, np.int64)
    if overflow:
        num = num_a if num_a < 0 else num_b if num_b < 0 else -max(num_a, 1)
        segs, counts[5] = np.zeros((0, SEGMENT_COLS)), 1
    else:
        num = num_a
        seg_id[inherit] = ta[inherit, 4].astype(np.int64)
        seg_id[fresh] = next_id + np.arange(int(fresh.sum()))          # the rank in ascending label order
        segs = np.stack([ta[:, 0], ta[:, 1], seg_id.astype(np.float64), inherit.astype(np.float64), ta[:, 5], ta[:, 9]], axis=1).reshape(L, SEGMENT_COLS)
        if L:
            _, seg = segments(labels)
            take = seg_id[seg] >= 0
            state[take] = seg_id[seg][take]
        counts[0:3] = link.sum(), inherit.sum(), fresh.sum()
        next_id = next_id + int(fresh.sum())
    obs = np.zeros((len(objects), OBS_COLS))
    for p, o in enumerate(objects):
        tid = -1
        if not overflow and o[22] > 0.0:
            with np.errstate(invalid="ignore"):
                c = find_segment(ta, L, F(o[1]))
            if c >= 0:
                tid = int(seg_id[c])
        obs[p] = [tid, gap, seconds, o[7], o[8], o[9], max(o[16], o[17]), min(o[16], o[17]), o[18], o[22], o[4], o[5], o[6]]
    counts[3], counts[4] = (obs[:, 0] >= 0).sum(), (obs[:, 0] < 0).sum()
    return dict(track_of_row=state, next_id=next_id, segments=segs, num=num, obs=obs, counts=counts)


def fit(obs, T, max_residual=MAX_RESIDUAL, min_speed=MIN_SPEED):
    """-> (tracks float64 [T, 16], counts int64 [5])"""
    obs = np.asarray(obs, np.float64).reshape(-1, OBS_COLS)
    out = np.zeros((T, TRACK_COLS))
    counts = np.zeros(FIT_COUNTS, np.int64)
    counts[0] = T
    for t in range(T):
        mine = [[float(x) for x in o] for o in obs if o[0] == float(t)]
        num, den, mask = [0.0, 0.0, 0.0], 0.0, 0
        sizes = [0.0, 0.0, 0.0, 0.0]
        for o in mine:
            s = o[2]
            for a in range(3):
                num[a] = num[a] + s * o[3 + a]
            den = den + s * s
            if 0.0 <= o[1] < 64.0:
                mask |= 1 << int(o[1])
            for j in range(4):
                sizes[j] = o[6 + j] if o[6 + j] > sizes[j] else sizes[j]
        v, worst, total = [0.0, 0.0, 0.0], 0.0, 0.0
        if mine:
            with np.errstate(all="ignore"):
                v = [float(np.float64(num[a]) / np.float64(den)) for a in range(3)]
            for o in mine:
                rx, ry = o[3] - o[2] * v[0], o[4] - o[2] * v[1]
                r2 = rx * rx + ry * ry
                worst = r2 if r2 > worst else worst
                total = total + r2
        speed = math.sqrt(v[0] * v[0] + v[1] * v[1])
        largest, rms = math.sqrt(worst), math.sqrt(total / len(mine)) if mine else 0.0
        observed = bool(mine)
        moving = observed and speed >= min_speed
        judged = bin(mask).count("1") >= 2
        consistent = judged and largest <= max_residual
        out[t] = [t, len(mine), float(mask), v[0], v[1], v[2], speed, largest, rms, moving, judged, consistent] + sizes
        counts[1:] += [observed, judged, consistent, moving]
    return out, counts

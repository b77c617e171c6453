"""The crafted inputs of the trust byte's tests (tests/test_trust.py on the CPU, tests/test_gpu_trust.py on the GPU): segment
tables as icpflow_nn_residual_segments and icpflow_sight_segments would leave them -- made in numpy, so that every threshold
can be hit exactly --, the per-row arrays, the pair rows, and a small frame pair for the end-to-end test.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_restatement as tr                # noqa: E402

F = np.float32
SKIP = (F(-1e8), F(-1.0))
SNAN, QNAN = np.uint32(0x7F812345), np.uint32(0x7FC12345)     # a signalling NaN and its quiet form
# what a segment's AFTER side can be: (name, good rows, sum of d) -- `good` None: drawn
MEANS = (("fits", None, 0.03), ("equal", 10, 1.0), ("above", None, 0.25), ("just above", 10, float(np.nextafter(1.0, 2.0))), ("no good row", 0, 0.0),
         ("far above", None, 1.7))
# ... and its AFTER far rows per code 0 .. 4 (outside, no return, seen through, at first return, behind)
FARS = (("seen through", (0, 0, 6, 2, 2)), ("lost from view", (2, 2, 1, 1, 3)), ("tie", (0, 0, 5, 0, 5)), ("no far row", (0, 0, 0, 0, 0)),
        ("at first return", (1, 0, 1, 8, 0)), ("excused tie", (0, 5, 4, 1, 0)), ("all seen", (0, 0, 9, 0, 0)), ("all behind", (0, 0, 0, 0, 7)))


def special_labels():
    """labels every larger table carries: both skip labels, 0.0 (rows come with -0.0 too), a negative one, an infinity, two NaNs"""
    return np.concatenate([np.array([SKIP[0], SKIP[1], 0.0, -7.5, np.inf], F), np.array([QNAN, 0xFFC00001], np.uint32).view(F)])


def labels_for(L, seed):
    """L distinct labels (by the table's key) in the table's order, the specials among them from L = 8 on"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(1, 3 * L + 8, dtype=F), (rng.integers(1, 1000, 8) + 0.5).astype(F)])
    lab = special_labels()[:L] if L < 8 else special_labels()
    rest = rng.choice(pool, L - len(lab), replace=False).astype(F)
    lab = np.concatenate([lab, rest])
    k = tr.key(lab)
    assert len(np.unique(k)) == L
    return lab[np.argsort(k, kind="stable")]


def tables(labels, seed, mean=None, far=None):
    """-> (resid float64 [L, 18], sight float64 [L, 24], what [L] of (mean name, far name)): every segment draws one of MEANS and
    one of FARS (or takes the named ones)"""
    rng = np.random.default_rng(seed)
    L = len(labels)
    resid, sight, what = np.zeros((L, 18)), np.zeros((L, 24)), []
    with np.errstate(invalid="ignore"):
        resid[:, 0] = sight[:, 0] = np.asarray(labels, F).astype(np.float64)
    for c in range(L):
        mname, good, total = MEANS[rng.integers(len(MEANS))] if mean is None else next(m for m in MEANS if m[0] == mean)
        fname, fars = FARS[rng.integers(len(FARS))] if far is None else next(f for f in FARS if f[0] == far)
        if good is None:
            good = int(rng.integers(1, 400))
            total = total * good * float(rng.uniform(0.8, 1.2))
        rows = good + int(rng.integers(0, 3))
        resid[c, 1] = sight[c, 1] = max(rows, sum(fars) + 2)
        resid[c, 2:10] = (good, good, good // 2, good, 0, 0, 0.02 * good, 0.001 * good)       # BEFORE: fits
        resid[c, 10:18] = (good, good // 2, good // 3, good // 2, 0, 0, total, total * total / max(good, 1))
        sight[c, 2], sight[c, 13] = good, good
        sight[c, 14:24:2] = np.asarray(fars) + 1
        sight[c, 15:24:2] = fars
        what.append((mname, fname))
    return resid, sight, what


def pair_rows(P, stride, labels, seed, listed_twice=True):
    """-> float32 [P, stride]: column 0 about half of `labels` (one of them twice from P = 2 on, -0.0 for 0.0), the rest labels
    no segment has; the other columns noise"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-5, 5, (P, stride)).astype(F)
    if P:
        lab = np.asarray(labels, F)
        some = lab[(rng.random(len(lab)) < 0.5) & ~np.isnan(lab)]        # (a NaN in the pair rows matches nothing)
        col = np.where(rng.random(P) < 0.6, rng.choice(some, P) if len(some) else F(-3e4), -(rng.integers(2, 9999, P).astype(F)) - F(0.25)).astype(F)
        col[col == 0.0] = F(-0.0)
        if listed_twice and len(some):           # (P = 1: that one row)
            col[0] = col[P - 1] = some[0] if some[0] != 0.0 else F(-0.0)
        rows[:, 0] = col
    return rows


def rows(n, labels, seed, codes=True, flow=True, far=0.1):
    """n source rows -> dict(after, flow, labels, d2, code): labels of the table, a few no table has, -0.0 and a signalling NaN
    where the table has 0.0 and its quiet form; d2 on either side of far2 and ON it; every code; bad rows (inf, NaN, 2e6) by
    the point and by the flow alone"""
    rng = np.random.default_rng(seed)
    lab = np.asarray(labels, F)
    after = rng.uniform(-60, 60, (n, 3)).astype(F)
    fl = rng.uniform(-1, 1, (n, 3)).astype(F) if flow else None
    mine = rng.choice(lab, n).astype(F) if len(lab) else np.full(n, 3.0, F)
    absent = rng.random(n) < 0.05
    mine[absent] = (-(rng.integers(2, 9999, int(absent.sum())).astype(F)) - F(0.75))
    zero = (mine == 0.0) & (rng.random(n) < 0.5)
    mine[zero] = F(-0.0)
    b = mine.view(np.uint32).copy()
    b[(b == QNAN) & (rng.random(n) < 0.5)] = SNAN
    mine = b.view(F)
    far2 = F(far) * F(far)
    pool = np.array([0.0, far2, np.nextafter(far2, F(1)), np.nextafter(far2, F(0)), 4.0, 0.25], F)
    d2 = pool[rng.integers(0, len(pool), n)]
    code = rng.integers(0, 5, n).astype(np.int32) if codes else None
    bad = np.flatnonzero(rng.random(n) < 0.04)
    specials = np.array([[np.inf, 0, 0], [0, np.nan, 0], [0, 0, 2e6], [1e8, 1e8, 1e8]], F)
    for k, i in enumerate(bad):
        if fl is not None and k % 2:
            fl[i] = specials[k % 4]            # a good point that the flow makes bad
        else:
            after[i] = specials[k % 4]
        if code is not None:
            code[i] = -2
    return dict(after=after, flow=fl, labels=mine, d2=d2, code=code)


TRUE_FLOW = (0.25, 0.125, 0.0)
MISFLOWED, OCCLUDED = 1.0, 4.0


def frame_pair():
    """A rigid frame pair of about 3 000 points seen from (0, 0, 0): six patches of 300 points facing the sensor at 20 m, every 60
    degrees (labels 0 .. 5), a ring of ground (label -1e8) and scattered noise (label -1); the destination is the source moved
    by TRUE_FLOW and the flow is TRUE_FLOW, but
        MISFLOWED  its flow ends 3 m nearer to the sensor: in free space, in front of the patch's own returns
        OCCLUDED   its destination surface is gone and a wall stands at 10 m between it and the sensor
    -> dict(points_src, points_dst, labels_src, labels_dst, flow, pairs [6, 10])"""
    rng = np.random.default_rng(23)
    up = np.array([0.0, 0.0, 1.0])
    pts, lab = [], []
    for k in range(6):
        a = 2 * np.pi * k / 6 + 0.2
        d, side = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
        lateral, height = rng.uniform(-1.0, 1.0, 300), rng.uniform(-0.5, 0.5, 300)
        pts.append(20.0 * d + lateral[:, None] * side + height[:, None] * up)
        lab.append(np.full(300, float(k)))
    az, h = rng.uniform(0, 2 * np.pi, 900), rng.uniform(5.0, 12.0, 900)
    pts.append(np.stack([h * np.cos(az), h * np.sin(az), np.full(900, -1.7)], axis=1))
    lab.append(np.full(900, -1e8))
    az, h = rng.uniform(0, 2 * np.pi, 300), rng.uniform(30.0, 50.0, 300)
    pts.append(np.stack([h * np.cos(az), h * np.sin(az), rng.uniform(2.0, 8.0, 300)], axis=1))
    lab.append(np.full(300, -1.0))
    src, labels = np.concatenate(pts).astype(F), np.concatenate(lab).astype(F)
    flow = np.tile(np.asarray(TRUE_FLOW, F), (len(src), 1))
    dst = src + flow
    away = (src / np.linalg.norm(src, axis=1, keepdims=True)).astype(F)
    flow[labels == MISFLOWED] -= F(3.0) * away[labels == MISFLOWED]
    keep = labels != OCCLUDED
    a = 2 * np.pi * OCCLUDED / 6 + 0.2
    d, side = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
    lateral, height = rng.uniform(-1.5, 1.5, 500), rng.uniform(-1.0, 1.0, 500)
    wall = (10.0 * d + lateral[:, None] * side + height[:, None] * up).astype(F)
    labels_dst = np.concatenate([labels[keep], np.full(len(wall), 77.0, F)])
    dst = np.concatenate([dst[keep], wall])
    order = rng.permutation(len(src))
    pairs = np.zeros((6, 10), F)
    pairs[:, 0] = pairs[:, 1] = np.arange(6)
    return dict(points_src=src[order], points_dst=dst, labels_src=labels[order], labels_dst=labels_dst, flow=flow[order], pairs=pairs)

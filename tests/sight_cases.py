"""The inputs of tests/test_gpu_sight.py that carry a condition of their own -- a condition the CPU suite asserts on the
restatement (tests/test_sight.py), so that the GPU test cannot pass on a scene that does not exercise what it names.  numpy
only.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sight_restatement as S             # noqa: E402

F = np.float32
SHAPES = tuple((W, H) for W in (4, 8, 1024) for H in (1, 2, 3, 64))
SIZES = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2049)
ORIGIN = (0.5, -0.25, -1.0)               # dyadic, and 8 tan_lo - 1, 8 tan_hi - 1 are floats for the default tangents: u = v - o is exact for the border points below
MARGIN_RANGES = (2.0, 7.3, 20.0, 61.7, 150.0)


def _up(x):
    return np.nextafter(F(x), F(np.inf))


def _down(x):
    return np.nextafter(F(x), F(-np.inf))


def border_points(v):
    """Points on the borders of the map of view `v`, as (name, point) pairs; u = point - origin has a horizontal distance of
    exactly 8 where the row matters, so that t = uz / 8 is exact.  tests/test_sight.py asserts what each of them meets."""
    lo, hi, o = v["tan_lo"], v["tan_hi"], v["o"].astype(np.float64)
    mid = F(F(lo + hi) / F(2))
    rmin, rmax = v["min_range"], v["max_range"]
    u = [("column 0", (8, 2.0 ** -10, 8 * mid)), ("column W - 1", (8, -2.0 ** -10, 8 * mid)), ("p rounds to 4", (8, -2.0 ** -25, 8 * mid)),
         ("quadrant 2", (-8, 2.0 ** -10, 8 * mid)), ("quadrant 3", (-8, -2.0 ** -10, 8 * mid)), ("ux = -0", (-0.0, 8, 8 * mid)),
         ("uy = -0", (8, -0.0, 8 * mid)), ("row 0", (8, 0, 8 * _up(lo))), ("t == tan_lo", (8, 0, 8 * lo)), ("below tan_lo", (8, 0, 8 * _down(lo))),
         ("row H - 1", (0, 8, 8 * _down(hi))), ("t == tan_hi", (0, 8, 8 * hi)), ("vertical axis", (0, 0, 5)), ("vertical axis, -0", (-0.0, 0.0, -5)),
         ("far corner", (-8, 0, 8 * _down(hi)))]
    for name, r in (("min_range", rmin), ("max_range", rmax)):
        for k, x in ((-2, _down(_down(r))), (-1, _down(r)), (0, r), (1, _up(r)), (2, _up(_up(r)))):
            u.append((f"rho {name} {k:+d}", (x, 0, 0)))
    return [(name, (np.asarray(p, np.float64) + o).astype(F)) for name, p in u]


def sweep(m, seed, v, bad=False):
    """m returns of a sweep seen from the view's origin: directions all around, elevations a little beyond the field of view,
    ranges from half the minimum to a little beyond 60 m (and a few beyond the maximum).  bad: NaN, Inf and pad rows among
    them."""
    rng = np.random.default_rng(seed)
    az = rng.uniform(0, 2 * np.pi, m)
    t = rng.uniform(float(v["tan_lo"]) - 0.05, float(v["tan_hi"]) + 0.05, m)
    h = rng.uniform(0.5 * float(v["min_range"]), 60.0, m)
    if m >= 8:
        h[rng.choice(m, max(m // 50, 1), replace=False)] = float(v["max_range"]) * 1.1
    p = (np.stack([h * np.cos(az), h * np.sin(az), h * t], axis=1) + v["o"].astype(np.float64)).astype(F)
    if bad and m:
        specials = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e8, 1e8, 1e8], [1.5e6, 0, 0], [0, -1000001.0, 0]], F)
        k = min(m, 2 * len(specials))
        p[rng.choice(m, k, replace=False)] = specials[rng.integers(0, len(specials), k)]
    return p


def queries(n, seed, v, target, bad=False):
    """n query rows and a flow: a third on a return of `target` (q + f = the return, up to a jitter of a margin or so), the
    rest anywhere a sweep could see or not.  bad: NaN, Inf and pad rows, and finite rows whose FLOW is infinite or takes them
    beyond 1e6 m (good rows that the flow makes bad).  -> (points, flow, rows the flow makes bad)"""
    rng = np.random.default_rng(seed)
    q = sweep(n, seed + 1, v).astype(np.float64)
    if len(target) and n:
        near = rng.random(n) < 1 / 3
        ok = S.good(target)
        if ok.any():
            pick = np.flatnonzero(ok)[rng.integers(0, int(ok.sum()), int(near.sum()))]
            q[near] = target[pick].astype(np.float64) * rng.uniform(0.97, 1.03, (int(near.sum()), 1))
    f = rng.uniform(-0.5, 0.5, (n, 3))
    q, f = (q - f).astype(F), f.astype(F)
    spoiled = np.zeros(0, np.int64)
    if bad and n:
        specials = np.array([[np.nan, 0, 0], [0, np.inf, 0], [1e8, 1e8, 1e8], [0, -1000001.0, 0]], F)
        k = min(n, 2 * len(specials))
        rows = rng.choice(n, k, replace=False)
        q[rows] = specials[rng.integers(0, len(specials), k)]
        if n >= 64:
            spoiled = np.setdiff1d(np.arange(7, n, 29), rows)[:6]
            f[spoiled[::2], 1] = np.inf
            f[spoiled[1::2], 0] = 2e6
    return q, f, spoiled


def one_pixel(v, count=5000, seed=3):
    """`count` targets inside ONE pixel of the view (around the direction (1, 0.5, 0) from the origin, ranges 5 .. 50 m, every
    range there twice, the nearest one four times), and a permutation of its rows"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(5.0, 50.0, (count - 1) // 2)
    d = np.array([1.0, 0.5, 0.0]) / np.hypot(1.0, 0.5)
    jitter = rng.uniform(-1e-5, 1e-5, (len(r), 3))
    p = (r[:, None] * (d + jitter) + v["o"].astype(np.float64)).astype(F)
    p = np.concatenate([p, p, p[[int(np.argmin(r))] * 2]])
    return p, rng.permutation(len(p))


def margins(v, ranges=MARGIN_RANGES):
    """Per range one target on the x axis of the view (its own pixel: the ranges go to different targets and are tested one
    at a time) and four queries on the same ray, found by search over neighbouring floats:
        0: the LOWEST x with fl(rho + thr) == n9        -> not seen through (at the first return)
        1: the float below it                           -> seen through
        2: the HIGHEST x with fl(rho - thr) == n9       -> at the first return
        3: the float above it                           -> behind
    -> [(target [1, 3], queries [4, 3])]; the view's origin must be (0, 0, 0)"""
    assert not v["o"].any()
    out = []
    for base in ranges:
        R = F(base)
        for _ in range(64):                               # the next target range for which both equalities exist
            n9 = np.sqrt(F(R * R))
            found = []
            for sign in (1, -1):
                x0 = F((float(n9) - sign * float(v["margin_abs"])) / (1.0 + sign * float(v["margin_rel"])))
                xs = x0 + np.arange(-256, 257).astype(F) * np.spacing(x0)
                xs = np.unique(xs.astype(F))
                rho = np.sqrt(xs * xs)
                thr = v["margin_abs"] + v["margin_rel"] * rho
                hit = np.flatnonzero((rho + thr if sign > 0 else rho - thr) == n9)
                if len(hit):
                    x = xs[hit[0]] if sign > 0 else xs[hit[-1]]
                    found += [x, _down(x) if sign > 0 else _up(x)]
            if len(found) == 4:
                break
            R = _up(R)
        assert len(found) == 4, base
        q = np.zeros((4, 3), F)
        q[:, 0] = found
        out.append((np.array([[R, 0, 0]], F), q))
    return out


# ---- the verdict ------------------------------------------------------------------------------------------------------------
PULLED, WALLED, FLUNG, UNSEEN = 2.0, 4.0, 6.0, 8.0
TRUE_FLOW = (0.25, 0.125, 0.0)


def verdict():
    """A rigid frame pair of about 3 000 points seen from (0, 0, 0): ten patches of 220 points facing the sensor at 20 m, every
    36 degrees (labels 0 .. 9), a ring of ground below them (label -1e8) and scattered noise (label -1); the destination is the
    source moved by TRUE_FLOW, and the flow is TRUE_FLOW but for
        PULLED  its flow ends 3 m nearer to the sensor: in front of the patch's own returns
        WALLED  its destination surface is gone and a wall stands at 10 m between it and the sensor
        FLUNG   its flow ends 230 m further out, beyond max_range
        UNSEEN  its destination surface is gone and nothing else lies on its rays
    -> (source, flow, labels, destination)"""
    rng = np.random.default_rng(17)
    pts, lab = [], []
    for k in range(10):
        a = 2 * np.pi * k / 10 + 0.2
        d, side = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
        lateral, height = rng.uniform(-1.0, 1.0, 220), rng.uniform(-0.5, 0.5, 220)
        pts.append(20.0 * d + lateral[:, None] * side + height[:, None] * np.array([0.0, 0.0, 1.0]))
        lab.append(np.full(220, float(k)))
    az, h = rng.uniform(0, 2 * np.pi, 600), rng.uniform(5.0, 12.0, 600)
    pts.append(np.stack([h * np.cos(az), h * np.sin(az), np.full(600, -1.7)], axis=1))
    lab.append(np.full(600, -1e8))
    az, h = rng.uniform(0, 2 * np.pi, 200), rng.uniform(30.0, 50.0, 200)
    pts.append(np.stack([h * np.cos(az), h * np.sin(az), rng.uniform(2.0, 8.0, 200)], axis=1))
    lab.append(np.full(200, -1.0))
    src, labels = np.concatenate(pts).astype(F), np.concatenate(lab).astype(F)
    flow = np.tile(np.asarray(TRUE_FLOW, F), (len(src), 1))
    dst = src + flow                                         # (the query's own fp32 addition: unspoiled rows land ON a return)
    away = (src / np.linalg.norm(src, axis=1, keepdims=True)).astype(F)
    flow[labels == PULLED] -= F(3.0) * away[labels == PULLED]
    flow[labels == FLUNG] += F(230.0) * away[labels == FLUNG]
    keep = ~np.isin(labels, (WALLED, UNSEEN))
    a = 2 * np.pi * 4 / 10 + 0.2
    d, side = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
    lateral, height = rng.uniform(-1.5, 1.5, 400), rng.uniform(-1.0, 1.0, 400)
    wall = 10.0 * d + lateral[:, None] * side + height[:, None] * np.array([0.0, 0.0, 1.0])
    dst = np.concatenate([dst[keep], wall.astype(F)])
    order = rng.permutation(len(src))
    return src[order], flow[order], labels[order], dst

"""A plain numpy restatement of the line-of-sight check (include/icpflow_hip.h, 8(h); csrc/sight.hpp, csrc/sight.hip): the
pixel map in float32 with every operation rounded by itself, the depth image with its 3 x 3 plane, the ray test, and the table
per segment by tests/table_restatement.py's label rule.  Everything here is meant to equal the kernels bit for bit; `exact_pixel`
is the same map in exact rationals, which the CPU tests compare the float32 map against.  Not a test module."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_restatement as tr           # noqa: E402

F = np.float32
EMPTY = np.uint32(0x7F800000)            # the bits of +inf
BAD, OUTSIDE, NO_RETURN, SEEN_THROUGH, AT_FIRST_RETURN, BEHIND = -2, 0, 1, 2, 3, 4
COLS, SIDE = 24, 11
START = dict(W=1024, H=64, tan_lo=-0.6, tan_hi=0.4, min_range=1.0, max_range=200.0, margin_abs=0.2, margin_rel=0.01)


def view(origin=(0.0, 0.0, 0.0), **params):
    """the parameters (START where not given) and the origin narrowed to float32 once, as the host side does it"""
    p = dict(START, **params)
    v = dict(W=int(p["W"]), H=int(p["H"]), o=np.asarray(origin, np.float64).astype(F))
    for k in ("tan_lo", "tan_hi", "min_range", "max_range", "margin_abs", "margin_rel"):
        v[k] = F(p[k])
    v["rs"] = F(F(v["H"]) / F(v["tan_hi"] - v["tan_lo"]))
    v["quarter"] = F(v["W"] // 4)
    return v


def good(points):
    """the residual's bad-row rule: every coordinate finite and within 1e6 m"""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(points, F).reshape(-1, 3)) <= F(1e6)).all(axis=1)


def pixel(v, points):
    """float32 [n,3] (good rows) -> (row, col int64 [n] -- -1, -1 OUTSIDE --, rho float32 [n], p, t float32 [n])"""
    q = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ux, uy, uz = q[:, 0] - v["o"][0], q[:, 1] - v["o"][1], q[:, 2] - v["o"][2]
        h2 = ux * ux + uy * uy
        d2 = h2 + uz * uz
        rho = np.sqrt(d2)
        s = np.abs(ux) + np.abs(uy)
        g = uy / s
        p = np.where(ux >= 0, np.where(uy >= 0, g, F(4) + g), F(2) - g).astype(F)
        colf = np.floor(p * v["quarter"])
        t = uz / np.sqrt(h2)
        rowf = np.floor((t - v["tan_lo"]) * v["rs"])
        inside = (s != 0) & (t >= v["tan_lo"]) & (t < v["tan_hi"]) & ~(rho < v["min_range"]) & ~(rho > v["max_range"])
    assert rho.dtype == F and p.dtype == F and t.dtype == F and colf.dtype == F and rowf.dtype == F
    col = np.where(inside, colf, 0).astype(np.int64)
    row = np.where(inside, rowf, 0).astype(np.int64)
    col[col >= v["W"]] = 0
    row[row >= v["H"]] = v["H"] - 1
    row[~inside], col[~inside] = -1, -1
    return row, col, rho, p, t


def spread(plane0):
    """plane 1: the minimum over the 3 x 3 pixels, columns modulo W, rows clipped"""
    H, W = plane0.shape
    cols = np.minimum(np.minimum(np.roll(plane0, 1, axis=1), plane0), np.roll(plane0, -1, axis=1))
    out = cols.copy()
    out[1:] = np.minimum(out[1:], cols[:-1])
    out[:-1] = np.minimum(out[:-1], cols[1:])
    return out


def build(v, target):
    """-> (image uint32 [2, H, W], info (bad targets, targets outside, occupied pixels))"""
    t = np.asarray(target, F).reshape(-1, 3)
    ok = good(t)
    row, col, rho, _, _ = pixel(v, t[ok])
    inside = row >= 0
    plane0 = np.full((v["H"], v["W"]), EMPTY, np.uint32)
    np.minimum.at(plane0, (row[inside], col[inside]), rho[inside].view(np.uint32))
    return np.stack([plane0, spread(plane0)]), (int((~ok).sum()), int((~inside).sum()), int((plane0 != EMPTY).sum()))


def query(v, image, points, flow=None):
    """-> (code int32 [n], near float32 [n] (+inf without a pixel), counts [6]: bad rows, then codes 0 .. 4)"""
    q = np.asarray(points, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if flow is not None:
            q = q + np.asarray(flow, F).reshape(-1, 3)
        ok = good(q)
        code = np.full(len(q), BAD, np.int32)
        near = np.full(len(q), np.inf, F)
        row, col, rho, _, _ = pixel(v, q[ok])
        inside = row >= 0
        n9 = np.full(len(row), np.inf, F)
        n9[inside] = image[1][row[inside], col[inside]].view(F)
        thr = v["margin_abs"] + v["margin_rel"] * rho
        assert thr.dtype == F
        c = np.where(rho + thr < n9, SEEN_THROUGH, np.where(rho - thr <= n9, AT_FIRST_RETURN, BEHIND))
        c = np.where(np.isinf(n9), NO_RETURN, c)
        c = np.where(inside, c, OUTSIDE)
    code[ok], near[ok] = c, n9
    return code, near, [int((code == k).sum()) for k in (BAD, 0, 1, 2, 3, 4)]


def far2(far):
    return F(F(far) * F(far))


def segments(v, image, before, after, flow, labels, d2_before=None, d2_after=None, far=0.1):
    """-> dict(labels float64 [L], label_bits, rows int64 [L], table float64 [L, 24], code_before, code_after int32 [n],
    info [12]: query's counts of the BEFORE side, then of the AFTER side)"""
    cb, _, nb = query(v, image, before)
    ca, _, na = query(v, image, after, flow)
    order, rows, label_bits = tr.table(np.asarray(labels, F).reshape(-1))
    L = len(rows)
    table = np.zeros((L, COLS))
    for c, (label, count, start) in enumerate(rows):
        mine = order[int(start): int(start) + int(count)]
        table[c, 0], table[c, 1] = label, count
        for at, code, d2 in ((2, cb, d2_before), (2 + SIDE, ca, d2_after)):
            is_far = np.zeros(len(mine), bool) if d2 is None else np.asarray(d2, F)[mine] > far2(far)
            table[c, at] = int((code[mine] >= 0).sum())
            for k in range(5):
                table[c, at + 1 + 2 * k] = int((code[mine] == k).sum())
                table[c, at + 2 + 2 * k] = int(((code[mine] == k) & is_far).sum())
    return dict(labels=table[:, 0].copy(), label_bits=label_bits, rows=table[:, 1].astype(np.int64), table=table, code_before=cb, code_after=ca,
                info=nb + na)


# ---- the same map in exact rationals (column and row only) --------------------------------------------------------------------
def exact_pixel(v, point):
    """One point (float32 coordinates, exact as rationals) through the map in exact arithmetic: -> (row, col, where) with
    `where` = the distance of (p W / 4, (t - tan_lo) rs) from the nearest pixel border, in pixels -- so that the caller can keep
    to points clear of borders, where rounding cannot change the floor.  t needs sqrt(h2): the row is decided by comparing
    squares (uz^2 against (lo + k / rs')^2 h2 with rs' = H / (tan_hi - tan_lo) exact), no square root taken.  None: OUTSIDE by
    the angles (the ranges are not looked at)."""
    o = [Fraction(float(x)) for x in v["o"]]
    ux, uy, uz = (Fraction(float(c)) - oc for c, oc in zip(point, o))
    s = abs(ux) + abs(uy)
    if s == 0:
        return None
    g = uy / s
    p = g if ux >= 0 and uy >= 0 else (4 + g if ux >= 0 else 2 - g)
    x = p * (v["W"] // 4)
    col = int(x // 1) % v["W"]
    lo, hi, H = Fraction(float(v["tan_lo"])), Fraction(float(v["tan_hi"])), v["H"]
    h2 = ux * ux + uy * uy

    def below(bound):                       # t < bound, with t = uz / sqrt(h2), h2 > 0
        if uz < 0:
            return bound >= 0 or uz * uz > bound * bound * h2
        return bound > 0 and uz * uz < bound * bound * h2

    if below(lo) or not below(hi):
        return None
    row = 0
    while row + 1 < H and not below(lo + (hi - lo) * (row + 1) / H):
        row += 1
    # the distance to the row's borders, in pixels, from a float64 tangent (a measure only, not a decision)
    t = float(uz) / float(h2) ** 0.5
    y = (t - float(lo)) * H / float(hi - lo)
    where = min(float(x - x // 1), float(1 - (x - x // 1)), y - np.floor(y), 1 - (y - np.floor(y)))
    return row, col, where

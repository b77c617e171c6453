"""Plain numpy restatement of the object boxes (icpflow_segment_boxes, icpflow_pair_objects; csrc/boxes.hip), written from
include/icpflow_hip.h, "8(j) object boxes": float32 with the exact fma32 of tests/sort_restatement.py for the projections,
float64 without fma for the centres and the objects.  Minima, maxima and counts do not depend on the order of the rows, so the
kernels' outputs equal these value for value (np.array_equal; the sign of a zero is the one thing left open).  Not a test
module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sort_restatement import fma32                 # noqa: E402

F = np.float32
BOX_COLS, OBJECT_COLS, TABLE_COLS = 16, 24, 9
INF = F(np.inf)


def directions(A=90):
    """the direction table utils_objects.box_directions builds: cos / sin of k (pi / 2) / A taken in float64, narrowed"""
    a = np.arange(A, dtype=np.float64) * (np.pi / 2) / A
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F)


def segments_of(num, Lmax):
    return 0 if num <= 0 else min(int(num), int(Lmax))


def segment_rows(row, n):
    """(start, count) of a table row as the kernels clip it to a cloud of n rows"""
    c, s = float(row[1]), float(row[2])
    if s >= 0.0 and s <= float(n) and c > 0.0:
        start = int(s)
        return start, (int(c) if c < float(n - start) else n - start)
    return 0, 0


def projections(points, order, row, n, dirs):
    """the good rows of one segment projected on every direction -> (u [g, A], v [g, A], z [g]) float32"""
    start, count = segment_rows(row, n)
    idx = np.asarray(order[start: start + count], np.int64)
    idx = idx[(idx >= 0) & (idx < n)]
    p = np.asarray(points, F).reshape(-1, 3)[idx]
    p = p[np.isfinite(p).all(axis=1)]
    with np.errstate(all="ignore"):
        x, y = (p[:, 0] - F(row[3]))[:, None], (p[:, 1] - F(row[4]))[:, None]
        c, s = dirs[None, :, 0], dirs[None, :, 1]
        u = _fma(y, s, x * c)
        v = _fma(y, c, -(x * s))
    return u, v, p[:, 2]


def _fma(a, b, c):
    """fma32, which is written for finite operands; where the plain float64 evaluation is not finite (a centroid that is NaN or
    infinite: its segment held such rows) that value is fmaf's too"""
    a, b, c = np.broadcast_arrays(a, b, c)
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    return np.where(np.isfinite(plain), fma32(a, b, c), plain)


def scores(u, v, delta):
    """per direction: (umin, umax, vmin, vmax, area) float32 and near (int)"""
    with np.errstate(all="ignore"):
        ulo, uhi = np.fmin.reduce(u, axis=0, initial=INF), np.fmax.reduce(u, axis=0, initial=-INF)
        vlo, vhi = np.fmin.reduce(v, axis=0, initial=INF), np.fmax.reduce(v, axis=0, initial=-INF)
        area = (uhi - ulo) * (vhi - vlo)
        side = np.fmin(np.fmin(uhi - u, u - ulo), np.fmin(vhi - v, v - vlo))
        near = (side <= F(delta)).sum(axis=0)
    return ulo, uhi, vlo, vhi, area, near


def pick(near, area):
    """the best direction: most near rows, then the smaller area, then the lower k -- the kernel's sequential comparison"""
    if not np.isnan(area).any():
        cand = np.flatnonzero(near == near.max())
        return int(cand[np.argmin(area[cand])])
    best = 0
    for k in range(1, len(near)):
        if near[k] > near[best] or (near[k] == near[best] and area[k] < area[best]):
            best = k
    return best


def segment_boxes(points, order, table, num, dirs, delta, Lmax=None):
    """-> float64 [L, 16], L = the segments the call writes (0 with num <= 0, at most Lmax)"""
    points = np.asarray(points, F).reshape(-1, 3)
    table = np.asarray(table, np.float64).reshape(-1, TABLE_COLS)
    dirs = np.asarray(dirs, F).reshape(-1, 2)
    n = len(points)
    L = segments_of(num, len(table) if Lmax is None else Lmax)
    out = np.zeros((L, BOX_COLS))
    for c in range(L):
        row = table[c]
        out[c, 0], out[c, 1], out[c, 3] = row[0], row[1], -1.0
        if row[0] < 0.0:
            continue
        u, v, z = projections(points, order, row, n, dirs)
        if len(z) == 0:
            continue
        ulo, uhi, vlo, vhi, area, near = scores(u, v, delta)
        k = pick(near, area)
        ck, sk = np.float64(dirs[k, 0]), np.float64(dirs[k, 1])
        with np.errstate(all="ignore"):
            um = (np.float64(ulo[k]) + np.float64(uhi[k])) * 0.5
            vm = (np.float64(vlo[k]) + np.float64(vhi[k])) * 0.5
            rx, ry = np.float64(F(row[3])), np.float64(F(row[4]))
            zlo, zhi = np.float64(z.min()), np.float64(z.max())
            out[c, 2:6] = len(z), k, near[k], np.float64(area[k])
            out[c, 6] = rx + (ck * um - sk * vm)
            out[c, 7] = ry + (sk * um + ck * vm)
            out[c, 8] = (zlo + zhi) * 0.5
            out[c, 9] = np.float64(uhi[k]) - np.float64(ulo[k])
            out[c, 10] = np.float64(vhi[k]) - np.float64(vlo[k])
            out[c, 11] = zhi - zlo
        out[c, 12:16] = ck, sk, zlo, zhi
    return out


def cluster_table(points, labels):
    """(order int64 [n], table float64 [L, 9]) as icpflow_cluster_table writes them, for the CPU tests: labels ascending with
    -0.0 and +0.0 one label (NaN labels are not built here), rows stable, the centroid the float32 mean (summed in float64 and
    narrowed: the tests that use it compare with the restatement alone), zeros for negative labels.  Extents are not filled."""
    points, labels = np.asarray(points, F).reshape(-1, 3), np.asarray(labels, F).reshape(-1) + F(0.0)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    unq, start, count = np.unique(labels[order], return_index=True, return_counts=True)
    table = np.zeros((len(unq), TABLE_COLS))
    table[:, 0], table[:, 1], table[:, 2] = unq, count, start
    for c in range(len(unq)):
        if unq[c] >= 0:
            with np.errstate(all="ignore"):
                table[c, 3:6] = points[order[start[c]: start[c] + count[c]]].astype(np.float64).mean(axis=0).astype(F)
    return order, table


def label_key(f):
    """csrc/labelkey.hpp's key of a float32 label (quieted first, as the box table's float64 column holds it)"""
    f = F(f)
    u = int(np.array(f, F).view(np.uint32))
    if f != f:
        u |= 0x00400000
    elif f == 0:
        u = 0
    k = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    return 0xfffffffe if k == 0xffffffff else k


def find_segment(boxes, L, label):
    keys = [label_key(F(boxes[c, 0])) for c in range(L)]
    want = label_key(label)
    lo, hi = 0, L
    while lo < hi:
        mid = (lo + hi) >> 1
        if keys[mid] < want:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < L and keys[lo] == want else -1


def pair_objects(boxes_src, num_src, boxes_dst, num_dst, pairs, T, seconds=0.1, min_speed=0.5, Lmax=None):
    """-> (objects float64 [P, 24], counts int64 [4])"""
    D = np.float64
    pairs = np.asarray(pairs, F)
    pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim == 2 else 2)
    P = len(pairs)
    T = np.asarray(T, F).reshape(P, 16)
    bs = np.asarray(boxes_src, D).reshape(-1, BOX_COLS)
    Ls = segments_of(num_src, len(bs) if Lmax is None else Lmax)
    bd = None if boxes_dst is None else np.asarray(boxes_dst, D).reshape(-1, BOX_COLS)
    Ld = 0 if bd is None else segments_of(num_dst, len(bd) if Lmax is None else Lmax)
    seconds, limit = D(seconds), D(min_speed) * D(min_speed)
    out, counts = np.zeros((P, OBJECT_COLS)), np.zeros(4, np.int64)
    with np.errstate(all="ignore"):
        for p in range(P):
            cs = find_segment(bs, Ls, pairs[p, 0])
            cd = find_segment(bd, Ld, pairs[p, 1]) if bd is not None else -1
            out[p, 0:4] = D(pairs[p, 0]), D(pairs[p, 1]), cs, cd
            counts[2] += cs < 0
            counts[3] += cd < 0
            if cs < 0 or not (bs[cs, 3] >= 0.0 and bs[cs, 2] > 0.0):
                continue
            b, m = bs[cs], T[p].astype(D)
            c = [b[6], b[7], b[8]]
            d = [(((m[4 * a] * c[0] + m[4 * a + 1] * c[1]) + m[4 * a + 2] * c[2]) + m[4 * a + 3]) - c[a] for a in range(3)]
            vel = [d[a] / seconds for a in range(3)]
            speed2 = vel[0] * vel[0] + vel[1] * vel[1]
            moving = bool(speed2 >= limit)
            ck, sk, du, dv = b[12], b[13], b[9], b[10]
            ex, ey = [ck, -sk, -ck, sk], [sk, ck, -sk, -ck]
            mq = 0
            if moving:
                best = ex[0] * d[0] + ey[0] * d[1]
                for q in range(1, 4):
                    dot = ex[q] * d[0] + ey[q] * d[1]
                    if dot > best:
                        best, mq = dot, q
            else:
                mq = 0 if du >= dv else 1
            counts[0] += 1
            counts[1] += moving
            out[p, 4:7], out[p, 7:10], out[p, 10:13] = c, d, vel
            out[p, 13:16] = speed2, float(moving), mq
            out[p, 16:19] = (dv if mq & 1 else du), (du if mq & 1 else dv), b[11]
            out[p, 19:21] = ex[mq], ey[mq]
            target = cd >= 0 and bd[cd, 3] >= 0.0 and bd[cd, 2] > 0.0
            gap = -1.0
            if target:
                gx, gy = (c[0] + d[0]) - bd[cd, 6], (c[1] + d[1]) - bd[cd, 7]
                gap = gx * gx + gy * gy
            out[p, 21:24] = gap, b[2], (bd[cd, 2] if target else 0.0)
    return out, counts

"""A plain numpy restatement of icpflow_nn_residual (include/icpflow_hip.h, 8(g)): brute force over all pairs in chunks of
queries, no grid.  Every operation is a float32 numpy operation on float32 arrays, so each is rounded by itself, in the order
the header states:

    q = p + f;  r2 = float32(r) * float32(r);  dx = q.x - t.x ...;  d2 = (dx * dx + dy * dy) + dz * dz;  hit = d2 <= r2

Per query the minimum d2 over the hits and the lowest target row that attains it (np.argmin returns the first minimum); no
hit: idx -1, d2 = r2.  A row with a non-finite coordinate or one beyond 1e6 m is bad: a bad target is never a neighbour, a bad
query (judged on q, or a group outside [0, G)) gets idx -2, d2 = r2 and enters no cell of the table.  The table per group:
good rows, hits, rows with d <= edge (d = sqrt(d2) in float32, widened; the edge in float64), and the sums of d and of d * d
(the exact float64 product) through math.fsum.

`exact_dyadic` is the same search in exact integer arithmetic for coordinates that are multiples of 1/16 inside +-64 m."""
import math

import numpy as np

FAR = np.float32(1e6)


def good_rows(x):
    with np.errstate(invalid="ignore"):
        return (np.abs(x) <= FAR).all(axis=1)          # (a NaN fails the comparison)


def radius2(radius):
    return np.float32(radius) * np.float32(radius)


def search(query, target, flow=None, radius=2.0, groups=None, n_groups=1, chunk_elems=1 << 18):
    """-> d2 float32 [n], idx int32 [n], info dict(bad_queries, bad_targets)"""
    p = np.ascontiguousarray(query, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
    n, m = len(p), len(t)
    with np.errstate(invalid="ignore", over="ignore"):
        q = p if flow is None else p + np.ascontiguousarray(flow, dtype=np.float32).reshape(-1, 3)
    r2 = radius2(radius)
    bad_q = ~good_rows(q)
    if groups is not None:
        g = np.asarray(groups).reshape(-1)
        bad_q |= (g < 0) | (g >= n_groups)
    good_t = good_rows(t)
    d2_out = np.full(n, r2, np.float32)
    idx_out = np.where(bad_q, -2, -1).astype(np.int32)
    rows = np.flatnonzero(~bad_q)
    step = max(1, chunk_elems // max(m, 1))
    if m:
        for a in range(0, len(rows), step):
            r = rows[a: a + step]
            with np.errstate(invalid="ignore", over="ignore"):
                dx = q[r, 0:1] - t[None, :, 0]
                dy = q[r, 1:2] - t[None, :, 1]
                dz = q[r, 2:3] - t[None, :, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            d2[:, ~good_t] = np.inf
            first = np.argmin(d2, axis=1)               # the first of equal minima: the lowest row
            best = d2[np.arange(len(r)), first]
            hit = best <= r2
            d2_out[r[hit]] = best[hit]
            idx_out[r[hit]] = first[hit]
    return d2_out, idx_out, dict(bad_queries=int(bad_q.sum()), bad_targets=int((~good_t).sum()))


def table(d2, idx, groups=None, n_groups=1, edges=()):
    """-> dict(rows, hits int64 [G], under int64 [G,E], dsum, ddsum float64 [G] through math.fsum)"""
    G, E = int(n_groups), len(edges)
    g = np.zeros(len(d2), np.int64) if groups is None else np.asarray(groups).reshape(-1).astype(np.int64)
    good = idx != -2
    d = np.sqrt(np.asarray(d2, np.float32)).astype(np.float64)      # float32 square root, correctly rounded, then widened
    out = dict(rows=np.zeros(G, np.int64), hits=np.zeros(G, np.int64), under=np.zeros((G, E), np.int64), dsum=np.zeros(G), ddsum=np.zeros(G))
    for k in range(G):
        mine = good & (g == k)
        out["rows"][k] = int(mine.sum())
        out["hits"][k] = int((mine & (idx >= 0)).sum())
        for e, edge in enumerate(edges):
            out["under"][k, e] = int((mine & (d <= float(edge))).sum())
        out["dsum"][k] = math.fsum(d[mine].tolist())
        out["ddsum"][k] = math.fsum((d[mine] * d[mine]).tolist())
    return out


def residual(query, target, flow=None, radius=2.0, groups=None, n_groups=1, edges=()):
    """-> (d2, idx, table dict, info dict): the whole call"""
    d2, idx, info = search(query, target, flow, radius, groups, n_groups)
    return d2, idx, table(d2, idx, groups, n_groups, edges), info


def table_words(tab):
    """the table dict in the kernel's int64 layout [G][E + 4] (sums as their bits)"""
    G, E = tab["under"].shape
    w = np.empty((G, E + 4), np.int64)
    w[:, 0], w[:, 1], w[:, 2:2 + E] = tab["rows"], tab["hits"], tab["under"]
    w[:, 2 + E], w[:, 3 + E] = tab["dsum"].view(np.int64), tab["ddsum"].view(np.int64)
    return w.reshape(-1)


# ---- exact integer arithmetic on dyadic clouds -------------------------------------------------------------------------------
SCALE = 16          # coordinates and flows are k / 16


def exact_dyadic(kq, kf, kt, radius):
    """kq, kf [n,3], kt [m,3]: integers, the coordinates times 16, with q = (kq + kf) / 16 and t inside +-64 m.  Every
    difference (|.| <= 2048), square (<= 2^22) and sum (<= 3 * 2^22 < 2^24) of the float32 computation is then exact, so
    d2 = D / 256 with D the int64 sum of squares, compared exactly against r2.  -> d2 float32 [n], idx int32 [n]"""
    kq, kt = np.asarray(kq, np.int64) + (0 if kf is None else np.asarray(kf, np.int64)), np.asarray(kt, np.int64)
    assert np.abs(kq).max(initial=0) <= 64 * SCALE and np.abs(kt).max(initial=0) <= 64 * SCALE
    r2 = float(radius2(radius))
    n = len(kq)
    d2_out, idx_out = np.full(n, np.float32(r2), np.float32), np.full(n, -1, np.int32)
    if len(kt) == 0:
        return d2_out, idx_out
    D = ((kq[:, None, :] - kt[None, :, :]) ** 2).sum(axis=2)         # int64, exact
    first = np.argmin(D, axis=1)
    best = D[np.arange(n), first]
    hit = best.astype(np.float64) / (SCALE * SCALE) <= r2           # both sides exact in float64
    d2_out[hit] = (best[hit].astype(np.float64) / (SCALE * SCALE)).astype(np.float32)   # < 2^24 / 256: exact in float32
    idx_out[hit] = first[hit]
    return d2_out, idx_out


def dyadic_clouds(count, seed=0):
    """`count` dyadic scenes (kq, kf, kt, radius): random clouds of mixed spread, clouds with duplicated targets, cubic
    lattices with the queries on lattice points and half way between them (ties), empty and single-point clouds"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(count):
        kind = c % 4
        radius = float(rng.choice([0.0625, 0.25, 0.5, 1.0, 2.0, 3.5]))
        if kind == 0:                                   # a random cloud, spread from dense to sparse
            span = int(rng.choice([8, 32, 200, 1000]))
            n, m = int(rng.integers(0, 40)), int(rng.integers(0, 60))
            kt = rng.integers(-span, span + 1, (m, 3))
            kq = rng.integers(-span, span + 1, (n, 3))
            kf = rng.integers(-8, 9, (n, 3))
        elif kind == 1:                                 # duplicated targets: the lowest row wins
            span = int(rng.choice([4, 16, 64]))
            base = rng.integers(-span, span + 1, (int(rng.integers(1, 12)), 3))
            kt = base[rng.integers(0, len(base), int(rng.integers(1, 50)))]
            kq = rng.integers(-span, span + 1, (int(rng.integers(1, 30)), 3))
            kf = rng.integers(-2, 3, kq.shape)
        elif kind == 2:                                 # a cubic lattice of pitch 2^k / 16, queries on and between its points
            pitch = int(rng.choice([2, 4, 16]))
            side = int(rng.integers(2, 5))
            ax = (np.arange(side) - side // 2) * pitch
            kt = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(side ** 3)]
            kq = kt[rng.integers(0, len(kt), 20)] + rng.choice([0, pitch // 2], (20, 3))
            kf = None
        else:                                           # the scene at the edge of the range, and the small ones
            m = int(rng.choice([0, 1, 2, 5]))
            kt = rng.choice([-1024, -1023, 1023, 1024, 0], (m, 3))
            kq = rng.choice([-1024, -1023, 1023, 1024, 0], (int(rng.integers(0, 6)), 3))
            kf = None
        kq, kt = np.clip(kq, -1024, 1024), np.clip(kt, -1024, 1024)
        if kf is not None:
            kf = np.clip(kq + kf, -1024, 1024) - kq
        out.append((kq.astype(np.int64), None if kf is None else kf.astype(np.int64), kt.astype(np.int64), radius))
    return out


def dyadic_floats(kq, kf, kt):
    f = lambda k: None if k is None else (np.asarray(k, np.float64) / SCALE).astype(np.float32)   # noqa: E731
    return f(kq), f(kf), f(kt)

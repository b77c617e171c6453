"""Seeded point sets for DBSCAN and the HDBSCAN spanning tree whose clusters are THIN (tests/test_cluster_shapes.py,
tests/test_gpu_cluster_shapes.py, tools/dbg/cluster_fuzz.py), and `hook_forest`, which counts what such an input asks of
cluster.hip's union-find.

The kernels hook every core point to its lowest core neighbour in SORTED order (a forest), and only edges that still cross
trees reach the lock-free unions.  A Gaussian blob is a handful of trees; a line that crosses many grid cells is hundreds.
Every generator works in float64 on integer multiples of its step, adds `offset`, casts to float32 [n, 3] at the end and
shuffles the rows when `shuffle` (a seed) is given."""
import itertools
from types import SimpleNamespace

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from oracle import cluster as oc

CELL_BITS = 21                        # cluster_util.hpp: kCellBits
FAR = (5000.0, -7000.0, 30.0)


def _finish(P, shuffle=None, offset=None, parts=None):
    """float64 [n, 3] -> float32 rows (moved by `offset`, "centre" = the bounding box's middle to the origin), shuffled by the
    seed `shuffle`; `parts` (boolean row sets) follow the rows."""
    P = np.asarray(P, np.float64)
    if isinstance(offset, str):
        assert offset == "centre"
        offset = -0.5 * (P.min(0) + P.max(0))
    if offset is not None:
        P = P + np.asarray(offset, np.float64)
    out = P.astype(np.float32)
    if shuffle is not None:
        perm = np.random.default_rng(shuffle).permutation(len(out))
        out = out[perm]
        parts = None if parts is None else [q[perm] for q in parts]
    return out if parts is None else (out, *parts)


def _xy(x, y):
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    return np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)


def comb(T=48, L=60, step=0.2, gap=0.6, shuffle=None, offset=None, parts=False):
    """T teeth along +x at y = t * gap, L points each, and a spine at x = L * step that joins their ends: one cluster at
    eps 0.25; without the spine exactly T.  parts: -> (points, spine rows as a mask)."""
    teeth = _xy(np.arange(L)[None, :] * step, np.arange(T)[:, None] * gap)
    k = int(round((T - 1) * gap / step))
    spine = _xy(L * step, np.arange(k + 1) * step)
    is_spine = np.r_[np.zeros(len(teeth), bool), np.ones(len(spine), bool)]
    res = _finish(np.concatenate([teeth, spine]), shuffle, offset, [is_spine])
    return res if parts else res[0]


def spiral(n, step=0.2, arm=0.75, shuffle=None, offset=None):
    """Archimedean spiral r = arm * theta / 2 pi, n points `step` apart along the arc (arms 3 eps apart at eps 0.25)."""
    a = arm / (2.0 * np.pi)
    s = np.arange(n) * step
    th = np.sqrt(2.0 * s / a)                                   # arc length ~ a theta^2 / 2
    for _ in range(60):                                          # Newton on s(theta) = a/2 (theta sqrt(1+theta^2) + asinh theta)
        f = 0.5 * a * (th * np.sqrt(1.0 + th * th) + np.arcsinh(th)) - s
        th = th - f / (a * np.sqrt(1.0 + th * th))
    return _finish(_xy(a * th * np.cos(th), a * th * np.sin(th)), shuffle, offset)


def snake(rows=30, L=50, step=0.2, gap=0.6, shuffle=None, offset=None):
    """Rows along x, linked at alternating ends by short runs along y (boustrophedon): one cluster at eps 0.25."""
    pieces = [_xy(np.arange(L)[None, :] * step, np.arange(rows)[:, None] * gap)]
    k = int(round(gap / step))
    for r in range(rows - 1):
        x = (L - 1) * step if r % 2 == 0 else 0.0
        pieces.append(_xy(x, r * gap + np.arange(1, k) * step))
    return _finish(np.concatenate(pieces), shuffle, offset)


def walls(k=6, shuffle=None, offset=None):
    """Wall c: x = 0.48 c, y = -2 ... 2 in steps of 0.05; one lone point between each two walls at (0.48 c + 0.24, 0, 0).
    Rows: the walls in DESCENDING c, then the lone points c = 0 ... k - 2, so that cluster ids run against the sort order.
    At eps 0.25, min_points 8: k clusters (wall c is cluster k - 1 - c), every lone point has 7 neighbours, is no core point
    and touches walls c and c + 1: it must take k - 2 - c, the lower id."""
    y = np.arange(-40, 41) * 0.05
    pieces = [_xy(0.48 * c, y) for c in range(k - 1, -1, -1)]
    pieces.append(_xy(0.48 * np.arange(k - 1) + 0.24, 0.0))
    return _finish(np.concatenate(pieces), shuffle, offset)


WALL_ROWS = 81


def dashes(n, run=50, shuffle=0, offset=None):
    """A line of n points 0.2 apart with a 1 m gap after every `run` points, shuffled: ceil(n / run) runs."""
    i = np.arange(n)
    return _finish(_xy(i * 0.2 + (i // run) * 0.8, 0.0), shuffle, offset)


def dust(side, shuffle=None, offset=None):
    """side x side x 2 lattice, 1 m apart: with min_points 1 every point is a cluster of its own."""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    return _finish(g.astype(np.float64), shuffle, offset)


def cells(points, eps):
    """cell_coord of cluster_util.hpp for every coordinate: cell = eps (1 + 2^-20), bias 2^20, clamped.  -> int64 [n, 3]"""
    inv = 1.0 / (float(eps) * (1.0 + 1.0 / float(1 << 20)))
    q = np.floor(np.asarray(points, np.float32)[:, :3].astype(np.float64) * inv) + float(1 << (CELL_BITS - 1))
    return np.clip(q, 1.0, float((1 << CELL_BITS) - 2)).astype(np.int64)


def keys(points, eps):
    c = cells(points, eps).astype(np.uint64)
    return (c[:, 0] << np.uint64(2 * CELL_BITS)) | (c[:, 1] << np.uint64(CELL_BITS)) | c[:, 2]


def _signed_perms(v):
    out = {tuple(s * c for s, c in zip(sg, pm)) for pm in itertools.permutations(v) for sg in itertools.product((1, -1), repeat=3)}
    return sorted(out)


def exact_pairs():
    """-> [(eps, points)] for eps = 7/32 and 3/8.  Rows 2 i and 2 i + 1 are a pair (p, p + v) with |v| = eps EXACTLY: v runs over
    the permutations and sign patterns of (2, 3, 6) / 32, resp. (1, 2, 2) / 8, every coordinate is a multiple of 1/32 below
    1024 (exact in float32, d^2 exact in fp64).  Every v is paired with every neighbour-cell offset t its signs allow: per
    axis p sits on the first or the last multiple of 1/32 inside its grid cell, whichever makes p + v land in cell + t.
    Cells of both signs, coordinates 0.0 and -0.0 included; pairs are 4.5 m apart along x."""
    out = []
    for eps, vs in ((7.0 / 32.0, [tuple(c / 32.0 for c in v) for v in _signed_perms((2, 3, 6))]),
                    (3.0 / 8.0, [tuple(c / 8.0 for c in v) for v in _signed_perms((1, 2, 2))])):
        cell = eps * (1.0 + 1.0 / float(1 << 20))
        combos = [(v, t) for v in vs for t in itertools.product((-1, 0, 1), repeat=3)
                  if any(t) and all(td == 0 or td == np.sign(c) for td, c in zip(t, v))]
        rows = []
        for i, (v, t) in enumerate(combos):
            m = (int(round((i - len(combos) // 2) * 4.5 / cell)), i % 5 - 2, i % 3 - 1)     # the cell of p, per axis
            p = []
            for md, c, td in zip(m, v, t):
                first = np.ceil(md * cell * 32.0)                 # first multiple of 1/32 at or above the cell's lower border
                high = (td == 1) or (td == 0 and c < 0)           # p + c crosses upwards / must not cross downwards
                pd = (first + 6.0 if eps < 0.25 else first + 11.0) / 32.0 if high else first / 32.0
                if pd == 0.0 and i % 2:
                    pd = -0.0
                p.append(pd)
            rows += [p, [a + b for a, b in zip(p, v)]]
        out.append((eps, np.asarray(rows, np.float64).astype(np.float32)))
    return out


def hook_forest(points, eps, min_points):
    """What dbscan_hook_kernel builds on this input, restated: key (cell_coord / pack_key), stable sort by key, every core
    point's parent = its lowest-position core neighbour below it (itself when there is none).  Describes the INPUT.
    -> trees, clusters, max_trees_in_cluster, contested (non-core points adjacent to >= 2 clusters), and per row: core,
    tree_of / cluster_of (-1 off the core points), contested_rows."""
    pts = np.asarray(points, np.float32)
    n = len(pts)
    assert np.isfinite(pts).all()
    order = np.argsort(keys(pts, eps), kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    pairs = oc.radius_pairs(pts, eps)
    core = np.bincount(pairs.reshape(-1), minlength=n) + 1 >= min_points
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    lo, hi = np.minimum(pos[cc[:, 0]], pos[cc[:, 1]]), np.maximum(pos[cc[:, 0]], pos[cc[:, 1]])
    parent = np.arange(n)                                   # over sorted positions
    np.minimum.at(parent, hi, lo)

    def comps(a, b):
        _, c = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
        c = np.where(core, c, -1)
        _, dense = np.unique(c[core], return_inverse=True)
        c[core] = dense
        return c

    tree_of = comps(order[np.arange(n)], order[parent])
    cluster_of = comps(cc[:, 0], cc[:, 1])
    n_trees, n_clusters = int(tree_of.max()) + 1 if core.any() else 0, int(cluster_of.max()) + 1 if core.any() else 0
    assert n_trees == int((core[order] & (parent == np.arange(n))).sum())
    per_cluster = np.bincount(np.unique(np.stack([cluster_of[core], tree_of[core]], 1), axis=0)[:, 0], minlength=n_clusters)
    touch = set()
    for a, b in ((0, 1), (1, 0)):
        sel = ~core[pairs[:, a]] & core[pairs[:, b]]
        touch |= set(zip(pairs[sel, a].tolist(), cluster_of[pairs[sel, b]].tolist()))
    adjacent = np.bincount(np.array([r for r, _ in touch], np.int64), minlength=n)
    return SimpleNamespace(trees=n_trees, clusters=n_clusters, max_trees_in_cluster=int(per_cluster.max()) if n_clusters else 0,
                           contested=int((adjacent >= 2).sum()), contested_rows=np.flatnonzero(adjacent >= 2), core=core,
                           tree_of=tree_of, cluster_of=cluster_of)

"""Seeded float32 scenes for the HDBSCAN spanning tree beyond one group of the chunk walk (csrc/hdbscan.hip), and their
restated trees (tests/hdbscan_restatement.py), cached per scene so that parametrised cases share them.

hdbscan.hip sorts the rows by an x-major cell key, cuts them into chunks of 64 and walks the chunks in groups of 64: up to
4 096 rows every search sees the whole cloud in its first step.  Each scene here is a function -> SimpleNamespace(points
[n, 3] float32, k, R, mask): R is the radius handed to `tree_within_radius` (None: `prim_tree`), mask a boolean row set or
None.  What a scene promises (group counts, shares of rows whose search crosses a group border, the rounds in which the
probe pass and the giant take part) is asserted with numbers by tests/test_hdbscan_restatement.py on the CPU;
tests/test_gpu_hdbscan_tree.py compares the device's tree with `tree(name)` edge for edge."""
from types import SimpleNamespace

import numpy as np

import hdbscan_restatement as hr

FAR = (5000.0, -7000.0, 30.0)
PLACES = {"origin": None, "far": FAR, "centred": "centre"}


def _finish(P, offset=None, shuffle=None):
    P = np.asarray(P, np.float64)
    if isinstance(offset, str):
        assert offset == "centre"
        offset = -0.5 * (P.min(0) + P.max(0))
    if offset is not None:
        P = P + np.asarray(offset, np.float64)
    out = P.astype(np.float32)
    if shuffle is not None:
        out = out[np.random.default_rng(shuffle).permutation(len(out))]
    return out


def _box(rng, n, size, origin=(0.0, 0.0, 0.0)):
    return rng.random((n, 3)) * np.asarray(size, np.float64) + np.asarray(origin, np.float64)


def _scene(points, k, R=None, mask=None):
    return SimpleNamespace(points=np.ascontiguousarray(points, dtype=np.float32), k=int(k), R=R, mask=mask)


# ------------------------------------------------------------------------------------------ seams of the chunk walk
SEAM_SIZES = {4096: 1, 4097: 2, 8192: 2, 8193: 3, 8900: 3}         # live rows -> groups of 64 chunks


def slab(n, place="origin", k=5, seed=0):
    """a lidar-crop-like slab of 30 x 20 x 2 m, uniformly random; 64 / 65 / 128 / 129 / 140 chunks"""
    rng = np.random.default_rng(1000 + n + seed)
    return _scene(_finish(_box(rng, n, (30.0, 20.0, 2.0)), PLACES[place]), k, R=3.0 if n < 6000 else 2.4)


# ------------------------------------------------------------------------------ where the x-termination can be wrong
def bar(axis, n=12300, k=4, seed=7):
    """200 m long and 1 m across.  axis 0: along x, the termination by the running x extreme fires on nearly every walk.
    axis 1 / 2: along y / z with EVERY x inside one 0.25 m cell ([0.01, 0.24]): the x gap never exceeds 0.23 m and the
    sort order inside the one x column (y cell, then z cell) is all that separates near from far."""
    rng = np.random.default_rng(seed + axis)
    P = _box(rng, n, (1.0, 1.0, 1.0))
    P[:, axis] *= 200.0
    if axis != 0:
        P[:, 0] = 0.01 + 0.23 * P[:, 0]
    return _scene(_finish(P), k, R=0.8)


def bridge(mirror=False, n_arc=8700, n_blob=300, k=4, seed=11):
    """A blob at x = 150 m and a crescent of 8 700 rows that opens towards it: rho(theta) = 145 + 20 theta^2 round the
    blob, |theta| <= 0.9, 0.2 m thick, so the crescent's row NEAREST the blob has the crescent's LOWEST x.  The one bridge edge (about
    145 m) joins the first group of 64 chunks with the last, across the whole chunk table; in the round that finds
    it the bound is far beyond every x gap, so no direction may end early.  mirror: x -> -x (the blob sorts first)."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(-0.9, 0.9, n_arc)
    rho = 145.0 + 20.0 * th * th + rng.uniform(0.0, 0.2, n_arc)
    arc = np.stack([150.0 - rho * np.cos(th), rho * np.sin(th), rng.uniform(0.0, 1.0, n_arc)], 1)
    blob = _box(rng, n_blob, (2.0, 2.0, 1.0), (150.0, -1.0, 0.0))
    P = np.concatenate([arc, blob])
    if mirror:
        P[:, 0] = -P[:, 0]
    return _scene(_finish(P, shuffle=seed), k)


def twin_slabs(n_each=4200, k=4, seed=13):
    """two slabs with the SAME x range, 150 m apart in y: the rows of both interleave through every x column of the
    sort, so every chunk column holds near and far rows and the x gap says nothing about the joining edge"""
    rng = np.random.default_rng(seed)
    P = np.concatenate([_box(rng, n_each, (30.0, 10.0, 2.0)), _box(rng, n_each, (30.0, 10.0, 2.0), (0.0, 150.0, 0.0))])
    return _scene(_finish(P, shuffle=seed), k)


def equal_x(planes=83, per=100, k=5, seed=17):
    """dyadic coordinates: `planes` x values 0.25 m apart (one per cell column), `per` rows on each (y, z multiples of 1 / 64 in 5 x 2 m).
    100 rows per plane and 64 per chunk: nearly every chunk border, and both group borders (positions 4 096 and
    8 192), lie INSIDE a run of exactly equal x."""
    rng = np.random.default_rng(seed)
    x = np.repeat(np.arange(planes) * 0.25, per)
    y = rng.integers(0, 5 * 64, planes * per) / 64.0
    z = rng.integers(0, 2 * 64, planes * per) / 64.0
    return _scene(_finish(np.stack([x, y, z], 1), shuffle=seed), k, R=0.9)


def folded_cell(chunks=130, k=4, seed=41):
    """8 320 rows inside ONE 0.25 m cell: every key is equal, the stable sort keeps the caller's order, and the caller's
    order is blocks of 64 rows, each block a thin x band (0.23 m / 130), the bands in shuffled order.  A chunk's OWN x range
    is then narrow and far from most queries, while the running extremes over the chunks behind it span the whole cell:
    only they may end a direction, and here they never do -- a row's neighbours sit in bands scattered over all 3 groups."""
    rng = np.random.default_rng(seed)
    band = np.repeat(rng.permutation(chunks), 64)
    P = 0.01 + 0.23 * rng.random((chunks * 64, 3))
    P[:, 0] = 0.01 + 0.23 * (band + rng.random(chunks * 64)) / chunks
    return _scene(_finish(P), k, R=0.04)


# ----------------------------------------------------------------------------------------- mostly empty chunk tables
def sparse_live(n_live, n=9000, k=4, seed=19):
    """n rows of which n_live take part, interleaved with masked rows and rows holding NaN / +Inf / -Inf in one
    coordinate: 141 chunks in 3 groups whatever n_live is, a partial last live chunk, all-dead chunks behind it"""
    rng = np.random.default_rng(seed + n_live)
    P = _box(rng, n, (30.0, 20.0, 2.0)).astype(np.float32)
    dead = rng.permutation(n)[n_live:]
    mask = np.ones(n, bool)
    kind = np.arange(len(dead)) % 4
    mask[dead[kind == 0]] = False                                       # finite, masked out
    for t, bad in ((1, np.nan), (2, np.inf), (3, -np.inf)):             # mask on, one coordinate not finite
        rows = dead[kind == t]
        P[rows, rows % 3] = bad
    return _scene(P, k, R=None if n_live < 1000 else 3.0 if n_live < 6000 else 2.4, mask=mask)


# ---------------------------------------------------------------------------------------- the top of the selection
def cloud(n, k, seed=23):
    """a slab at the slabs' density; 4 200 rows are two groups"""
    rng = np.random.default_rng(seed + n)
    s = (n / 4200.0) ** 0.5
    return _scene(_finish(_box(rng, n, (30.0 * s, 20.0 * s, 2.0))), k)


def copies(m, others=500, k=64, seed=29):
    """m copies of one point among `others`: with k = 64 the copies' core distance is 0 exactly for m >= 64"""
    rng = np.random.default_rng(seed + m)
    P = _box(rng, others, (6.0, 6.0, 2.0))
    return _scene(_finish(np.concatenate([P, np.repeat(P[:1] + 0.5, m, 0)]), shuffle=seed), k)


# ------------------------------------------------------------------------------------- ties decided by caller rows
def lattice(shuffle=None, dims=(24, 24, 8), step=0.25, k=7):
    """a dyadic lattice, every weight tied many times over; in meshgrid order the caller rows ARE the sorted order"""
    g = np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing="ij"), -1).reshape(-1, 3)
    return _scene(_finish(g * step, shuffle=shuffle), k)


# ----------------------------------------------------------------------------- the 1024-thread scan of chunk extremes
def wide(dims=(82, 80, 10), h=0.3, k=3, seed=31):
    """65 600 rows = 1 025 chunks = 17 groups: hdb_chunk_runs_kernel takes two chunks per thread and threads 513 ... 1023
    none.  One row per cell of a lattice of step h, jittered by +-0.3 h: neighbours in adjacent cells are at most 1.8 h
    apart, so R = 2.1 h certifies with about a million pairs."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing="ij"), -1).reshape(-1, 3)
    return _scene(_finish((g + rng.uniform(-0.3, 0.3, g.shape)) * h, shuffle=seed), k, R=2.1 * h)


SCENES = {f"slab_{n}_{place}": (lambda n=n, place=place: slab(n, place)) for n in SEAM_SIZES for place in PLACES}
SCENES.update({
    "bar_x": lambda: bar(0), "bar_y": lambda: bar(1), "bar_z": lambda: bar(2),
    "bridge": lambda: bridge(), "bridge_mirrored": lambda: bridge(mirror=True),
    "twin_slabs": twin_slabs, "equal_x": equal_x, "folded_cell": folded_cell,
    "sparse_100": lambda: sparse_live(100), "sparse_4097": lambda: sparse_live(4097), "sparse_8193": lambda: sparse_live(8193),
    "copies_70": lambda: copies(70), "copies_63": lambda: copies(63),
    "rows_64_k64": lambda: cloud(64, 64), "rows_65_k64": lambda: cloud(65, 64),
    "lattice_in_order": lambda: lattice(), "lattice_shuffled": lambda: lattice(shuffle=37),
    "wide_65600": wide,
})
SCENES.update({f"cloud_{n}_k{k}": (lambda n=n, k=k: cloud(n, k)) for n in (700, 4200) for k in (1, 2, 63, 64)})

_made, _trees = {}, {}


def scene(name):
    if name not in _made:
        _made[name] = SCENES[name]()
    return _made[name]


def live_rows(sc):
    ok = np.isfinite(sc.points).all(1)
    return np.flatnonzero(ok if sc.mask is None else ok & sc.mask)


def tree(name):
    """-> (lo, hi, w2, core2 [n] with NaN on rows that take no part) of the scene's restated tree, in caller rows, sorted by
    (lo, hi); computed once"""
    if name not in _trees:
        sc = scene(name)
        rows = live_rows(sc)
        sub = sc.points[rows]
        a, b, w2, c2 = hr.prim_tree(sub, sc.k) if sc.R is None else hr.tree_within_radius(sub, sc.k, sc.R)
        core2 = np.full(len(sc.points), np.nan)
        core2[rows] = c2
        _trees[name] = (rows[a], rows[b], w2, core2)          # rows is increasing: (lo, hi) order is kept
    return _trees[name]

"""The volumes of tests/test_peak_restatement.py (CPU: every case is what its name says) and tests/test_gpu_peaks.py (GPU: the
kernel on them).  A case is a dict: name, vol int64 [B, Lx, Ly, Lz], ks, k, form ("lds" / "global"), and what its builder knows about
it (meta).  Everything is generated from fixed seeds; nothing here needs a GPU.  Not a test module."""
import functools

import numpy as np

LDS_BINS = 150 * 1024 // 12          # three uint32 volumes in 150 KiB of LDS: 12800 bins
LIST = 512                           # kPeakList (csrc/hist.hip)
BIG, SMALL = 100, 50                 # the two values of a window-face pair (+ the pair's number: no two volumes alike)


def form(shape):
    return "lds" if int(np.prod(shape)) <= LDS_BINS else "global"


def z_branch(shape, ks):
    """Which branch of the LDS form's fused fill + z pass a shape reaches (csrc/hist.hip, kFillZ)."""
    r, Lz = (ks - 1) // 2, shape[2]
    if form(shape) == "global":
        return "global loop"
    if Lz == 3 and r >= 2:
        return "column of 3"
    return "whole column" if Lz <= r + 1 else "general loop"


def _case(name, vol, ks, k, **meta):
    vol = np.ascontiguousarray(vol, np.int64)
    assert vol.ndim == 4 and len(vol) >= 3, "B = 3 at least: the first and the last pair differ"
    return dict(name=name, vol=vol, ks=ks, k=k, shape=vol.shape[1:], form=form(vol.shape[1:]), **meta)


# ---------------------------------------------------------------------------------------------------------------------------------
# window faces: two distinct values on a background of 0, one pair per volume
# ---------------------------------------------------------------------------------------------------------------------------------
FACE_SHAPES = [((13, 12, 3), 11),                                   # z: the column of 3; y and x: lines
               ((13, 12, 6), 11),                                   # Lz = radius + 1: the whole column, rightly
               ((13, 12, 7), 11), ((12, 13, 11), 11),               # Lz = radius + 2 and 2 radius + 1
               ((9, 10, 12), 11),                                   # Lz = 2 radius + 2
               ((6, 5, 2), 3), ((5, 6, 3), 3), ((6, 7, 4), 3),      # radius 1: Lz = r + 1, r + 2 = 2 r + 1, 2 r + 2
               ((7, 6, 3), 5), ((7, 8, 4), 5), ((8, 7, 5), 5), ((7, 8, 6), 5),      # radius 2: the column of 3, r + 2, 2 r + 1, 2 r + 2
               ((9, 8, 4), 7), ((8, 9, 5), 7), ((9, 10, 7), 7), ((10, 9, 8), 7),    # radius 3: r + 1, r + 2, 2 r + 1, 2 r + 2
               ((30, 31, 14), 11), ((30, 31, 14), 7)]               # global scratch


@functools.lru_cache(maxsize=None)
def faces(shape, ks):
    """For every axis and both directions, a larger value with a smaller one `radius` away (suppressed) and `radius + 1` away (it
    survives), the pair at the first rows of the axis, at its last rows and inside; on an axis shorter than that, the pair as far
    apart as the axis allows.  One pair over the box's corner (radius, radius, radius): suppressed.  meta["pairs"]: per volume
    (axis, direction, distance, flat index of the larger, of the smaller, survives)."""
    r = (ks - 1) // 2
    mid = [n // 2 for n in shape]
    pairs = []
    for axis in range(3):
        n = shape[axis]
        dists = [d for d in (r, r + 1) if d <= n - 1] or [n - 1]
        for d in dists:
            starts = sorted({0, n - 1 - d, (n - 1 - d) // 2} if n - 1 - d >= 2 else {0, n - 1 - d})
            for start in starts:
                for direction in (+1, -1):
                    lo, hi = list(mid), list(mid)
                    lo[axis], hi[axis] = start, start + d
                    big, small = (lo, hi) if direction > 0 else (hi, lo)      # +1: the smaller one lies above the larger
                    pairs.append((axis, direction, d, tuple(big), tuple(small), d > r))
    if all(n >= r + 1 for n in shape):
        for direction in (+1, -1):
            lo, hi = [0, 0, 0], [r, r, r]
            big, small = (lo, hi) if direction > 0 else (hi, lo)
            pairs.append((3, direction, r, tuple(big), tuple(small), False))
            if shape[0] >= r + 2:                                  # ... and one step beyond the corner along x: outside the box
                hi2 = [r + 1, r, r]
                big, small = (lo, hi2) if direction > 0 else (hi2, lo)
                pairs.append((3, direction, r + 1, tuple(big), tuple(small), True))
    vol = np.zeros((len(pairs),) + tuple(shape), np.int64)
    meta = []
    for p, (axis, direction, d, big, small, survives) in enumerate(pairs):
        vol[(p,) + big], vol[(p,) + small] = BIG + p, SMALL + p
        meta.append((axis, direction, d, int(np.ravel_multi_index(big, shape)), int(np.ravel_multi_index(small, shape)), survives))
    return _case(f"faces {shape} ks{ks}", vol, ks, 8, pairs=meta, z_branch=z_branch(shape, ks))


def faces_parts(shape, ks):
    """faces(shape, ks) as the GPU file uploads it: a global-scratch shape in batches of 16 volumes at most."""
    c = faces(shape, ks)
    if c["form"] == "lds":
        return [c]
    return [_case(f"{c['name']} part {at // 16}", c["vol"][at: at + 16], ks, 8, pairs=c["pairs"][at: at + 16], z_branch=c["z_branch"])
            for at in range(0, len(c["vol"]), 16)]


@functools.lru_cache(maxsize=None)
def hand():
    """1 x 5 x 5 x 3, kernel_size 3, k = 2: h[2, 2, 0] = 5 and h[2, 2, 2] = 9 are two bins apart, radius 1: both survive.  Two more
    volumes so that the batch's ends differ: the same two values exchanged, and the 9 next to the 5 (the 5 is suppressed)."""
    vol = np.zeros((3, 5, 5, 3), np.int64)
    vol[0, 2, 2, 0], vol[0, 2, 2, 2] = 5, 9
    vol[1, 2, 2, 0], vol[1, 2, 2, 2] = 9, 5
    vol[2, 2, 2, 0], vol[2, 2, 2, 1] = 5, 9
    return _case("hand 5x5x3 ks3", vol, 3, 2, want_votes=[[9, 5], [9, 5], [9, 0]], want_idx=[[38, 36], [36, 38], [37, 0]])


# ---------------------------------------------------------------------------------------------------------------------------------
# permutation volumes: whether the second to eighth largest value survives depends on exact window extents
# ---------------------------------------------------------------------------------------------------------------------------------
PERMUTATION_SHAPES = [((13, 12, 9), 11, 64), ((13, 12, 7), 11, 64), ((12, 13, 11), 11, 64), ((9, 8, 3), 3, 64), ((8, 9, 5), 7, 64),
                      ((7, 6, 8), 5, 64), ((23, 25, 3), 11, 64), ((30, 31, 14), 11, 16), ((30, 31, 14), 7, 16)]


# (a seed is a property of the case: one under which some face of the window, moved by one step, changes no pair of the batch is
# replaced by the next one -- tests/test_peak_restatement.py asserts the condition, on the CPU, from the restatement alone)
PERMUTATION_RESEED = {((13, 12, 7), 11): 1}


def _permutations(shape, B, seed, crowd=0):
    """B random permutations of 1 .. L.  crowd = edge > 0: the 24 largest values of each volume are exchanged into a random box of
    that edge -- in a volume of thirteen thousand bins the largest eight of a uniform permutation seldom lie within a window of one
    another, and then no face of the window decides anything."""
    rng = np.random.default_rng(seed)
    L = int(np.prod(shape))
    vol = np.stack([rng.permutation(L) + 1 for _ in range(B)]).astype(np.int64)
    for b in range(B if crowd else 0):
        corner = [int(rng.integers(0, n - min(crowd, n) + 1)) for n in shape]
        cells = np.stack(np.meshgrid(*[c + np.arange(min(crowd, n)) for c, n in zip(corner, shape)], indexing="ij"), -1).reshape(-1, 3)
        to = np.ravel_multi_index(cells[rng.choice(len(cells), 24, replace=False)].T, shape)
        for v, f in zip(range(L, L - 24, -1), to):                 # exchange value v with whatever sits at f
            g = int(np.flatnonzero(vol[b] == v)[0])
            vol[b, g], vol[b, f] = vol[b, f], vol[b, g]
    return vol.reshape((B,) + tuple(shape))


@functools.lru_cache(maxsize=None)
def permutation(shape, ks, B):
    seed = 7000 + 100 * shape[0] + 10 * shape[1] + shape[2] + ks + 100000 * PERMUTATION_RESEED.get((shape, ks), 0)
    crowd = 2 * ks if form(shape) == "global" else 0
    return _case(f"permutation {shape} ks{ks}", _permutations(shape, B, seed, crowd), ks, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# line segments (kernel_size 11, LDS): Ly and Lx on both sides of the seams of the 11-bin segments
# ---------------------------------------------------------------------------------------------------------------------------------
LINE_SHAPES = [(10, 34, 3), (11, 33, 3), (12, 23, 3), (21, 22, 3), (22, 21, 3), (23, 12, 3), (33, 11, 3), (34, 10, 3),
               (12, 34, 31)]                                        # 12 x 31 x 4 = 1488 items in the y pass, 34 x 31 x 2 = 2108 in the x pass


def line_items(shape):
    """(items of the y pass, of the x pass): a thread takes one segment of 11 outputs of one line."""
    Lx, Ly, Lz = shape
    return Lx * Lz * -(-Ly // 11), Ly * Lz * -(-Lx // 11)


@functools.lru_cache(maxsize=None)
def lines(shape):
    B = 16 if int(np.prod(shape)) < 4096 else 4
    return _case(f"lines {shape} ks11", _permutations(shape, B, 9000 + 100 * shape[0] + shape[1]), 11, 8, items=line_items(shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# the survivors' list: exactly n positive survivors, n around k and around the list's 512 places
# ---------------------------------------------------------------------------------------------------------------------------------
LIST_SHAPE = (41, 41, 3)
LIST_L = 41 * 41 * 3
LIST_COUNTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 511, 512, 513, 600, LIST_L]


@functools.lru_cache(maxsize=None)
def survivors_ks1(n):
    """kernel_size 1: every positive bin survives.  n <= 7: the positive bins are the flat indices 0 .. n - 1 (the zero-vote fill
    has to step over all of them).  Otherwise they are spread over the volume, and the eight largest sit at the highest flat
    indices.  Volume 0: equal votes and eight larger ones; 1: all equal (the tie rule decides); 2: ascending with the index."""
    L = LIST_L
    rng = np.random.default_rng(100 + n)
    vol = np.zeros((3, L), np.int64)
    if n <= 7:
        at = np.arange(n)
    elif n == L:
        at = np.arange(L)
    else:
        at = np.sort(np.concatenate([rng.choice(L - 64, n - 8, replace=False), L - 1 - 5 * np.arange(8)]))
    if n:
        vol[0, at] = 3
        vol[0, at[-8:]] = 10 + np.arange(len(at[-8:]))
        vol[1, at] = 4
        vol[2, at] = 1 + np.arange(n)
    return _case(f"list ks1 n={n}", vol.reshape((3,) + LIST_SHAPE), 1, 8, n=n)


@functools.lru_cache(maxsize=None)
def survivors_ks11(n):
    """kernel_size 11: a run of equal votes from flat index 0 (equal neighbours all survive) plus, from n = 8 on, eight isolated
    larger votes in the rows x = 34 and x = 40 -- the highest flat indices of the positive bins, more than a window away from the
    run and from one another.  n <= 7: the run is the flat indices 0 .. n - 1, and bin n holds a smaller positive vote that the
    run suppresses: the fill must hand it out as a ZERO vote.  n = L: the plateau."""
    L = LIST_L
    vol = np.zeros((3, L), np.int64)
    iso = [np.ravel_multi_index((40, y, 2), LIST_SHAPE) for y in (40, 34, 28, 22, 16, 10, 4)] + [np.ravel_multi_index((34, 40, 2), LIST_SHAPE)]
    iso = np.sort(np.asarray(iso))
    for b in range(3):
        if n == L:
            vol[b] = (3, 1, 2 ** 24 - 1)[b]
        elif n <= 7:
            vol[b, :n] = 3 + b
            if n:
                vol[b, n] = 1 + b                                   # (positive, not surviving)
        else:
            vol[b, :n - 8] = 3 + b
            vol[b, iso] = 10 * (b + 1) + np.random.default_rng(b).permutation(8)
    return _case(f"list ks11 n={n}", vol.reshape((3,) + LIST_SHAPE), 11, 8, n=n)


# ---------------------------------------------------------------------------------------------------------------------------------
# the seam between the LDS form and the global one
# ---------------------------------------------------------------------------------------------------------------------------------
SEAM_SHAPES = [(64, 50, 4), (251, 17, 3)]                          # 12800 bins: the largest LDS volume; 12801: global


@functools.lru_cache(maxsize=None)
def seam(shape, ks, kind):
    if kind == "permutation":
        vol = _permutations(shape, 3, 500 + shape[0] + ks)
    else:
        vol = np.broadcast_to(np.array([3, 1, 7], np.int64).reshape(3, 1, 1, 1), (3,) + tuple(shape))
    return _case(f"seam {shape} ks{ks} {kind}", vol, ks, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pipeline's instantiation: uint32 counters, the fused decode
# ---------------------------------------------------------------------------------------------------------------------------------
U32_SHAPES = [((6, 5, 7), 3), ((5, 9, 11), 11), ((11, 7, 9), 7), ((9, 6, 8), 5), ((41, 40, 3), 11)]       # Lx != Ly != Lz; Lz in 7 .. 11 too
LARGE = [2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]


def edges(shape):
    """Bin edges that differ per axis and per bin: an index mix-up cannot cancel."""
    return tuple(np.float32(1000 * (a + 1)) + np.arange(n, dtype=np.float32) for a, n in enumerate(shape))


SHIFT = 0.25


@functools.lru_cache(maxsize=None)
def large_votes(ks):
    """Votes that float32 cannot tell apart (2^24 and 2^24 + 1 round to the same float, 2^24 + 2 and 2^24 + 3 to neighbours under
    round-to-even), votes around the sign bit and the largest ones.  kernel_size 1: all survive and only the order is asked;
    kernel_size 3: they sit next to one another along z, y and x in turn, so the window compares them too.  (The vote 2^32 - 1
    never sits in bin 0: its key there, all ones, is the selection's "nothing taken yet".)"""
    shape = (6, 5, 7)
    vol = np.zeros((3,) + shape, np.int64)
    rng = np.random.default_rng(31)
    for b in range(3):
        v = np.asarray(LARGE, np.int64)[rng.permutation(len(LARGE))]
        for j, val in enumerate(v):
            p = [1, 1, 1]
            p[(2, 1, 0)[b]] += j % 3                               # three in a row along one axis ...
            p[(0, 2, 1)[b]] = 2 * (j // 3)                         # ... the rows two apart (outside a window of 3)
            vol[(b,) + tuple(p)] = val
        vol[b][vol[b] == 0] = rng.choice(np.arange(1, 1000), int((vol[b] == 0).sum()), replace=False)      # (distinct)
        assert vol[b].ravel()[0] != 2 ** 32 - 1
    return _case(f"large votes ks{ks}", vol, ks, 8)

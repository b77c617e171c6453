"""The inputs of tests/test_gpu_tables.py, plain numpy.  What every input was built for -- the number of distinct labels, the
chunk count of every M, the 64 different labels of a scatter round, the home slots of the hash cases -- is asserted on the CPU in
tests/test_table_restatement.py: conditions on the inputs, not measurements of the kernels."""
import functools
import itertools

import numpy as np

import table_restatement as tr

F = np.float32
LMAX = 4096
SEAM_M = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 7680, 8191, 8192, 8193, 16384, 16385]
SEAM_CHUNKS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3, 15, 16, 16, 17, 32, 33]
LABEL_COUNTS = [1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3000, 4095, 4096]
OVERFLOWS = [(2, 1), (65, 64), (513, 512), (1025, 1024), (4097, 4096)]
PAIR_M = [(1, 1), (512, 1), (513, 512), (1, 513), (8193, 700), (700, 8193)]
SEVEN = np.array([-1e8, -1.0, -0.5, 0.25, 1.0, 2.5, 7.0], F)
RUN_CYCLE = np.array([4.0, -1.0, 2.5, 4.0, 0.0], F)      # a label per 256 rows: 4.0 comes back in both halves of a chunk
STAT_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 70000]
STAT_CENTRES = {"origin": (0.0, 0.0, 0.0), "3 km": (3000.0, -7000.0, 30.0), "+1e6 m": (1e6, 1e6, 1e6), "-1e6 m": (-1e6, -1e6, -1e6)}
# full extents of the boxes (multiples of 0.5: the corners centre +- e / 2 are float32 numbers at 1e6 m, where a step is 1 / 16):
# the six orders of three different extents, two equal (the pair first, last and apart), three equal
STAT_BOXES = [p for p in itertools.permutations((1.0, 2.0, 4.5))] + [(2.0, 2.0, 5.0), (5.0, 2.0, 2.0), (2.0, 5.0, 2.0), (3.0, 3.0, 3.0)]
DENSE_HOME = 7679      # the 1024 / 1025 labels of one home slot: their chain runs from here over the wrap at slot 8191


def distinct(L):
    """L different labels of alternating sign, so that the ascending order is not the order of arrival: 1, -1, 2, -2, ..."""
    j = np.arange(L)
    return ((j // 2 + 1) * np.where(j % 2 == 0, 1.0, -1.0)).astype(F)


def seam_patterns(M, seed=0):
    """-> {name: labels [M]}"""
    rng = np.random.default_rng(seed + M)
    i = np.arange(M)
    out = {"one label": np.full(M, 3.0, F),
           "two alternating": np.where(i % 2 == 0, 5.0, -2.0).astype(F),
           "seven iid": SEVEN[rng.integers(0, 7, M)],
           "sorted runs": np.sort(rng.integers(-3, 34, M)).astype(F),
           "runs of 256": RUN_CYCLE[(i // 256) % len(RUN_CYCLE)]}
    if M <= LMAX:
        out["every row its own"] = distinct(M)[rng.permutation(M)]
    return out


def counted(L, seed=0):
    """L distinct labels with 1 - 4 rows each, shuffled"""
    rng = np.random.default_rng(1000 + seed + L)
    lab = np.repeat(distinct(L), rng.integers(1, 5, L))
    return lab[rng.permutation(len(lab))]


def small_cloud():
    """five labels on 40 rows, for Lmax in 1, 7, 512, 4096 (Lmax = 1 overflows)"""
    rng = np.random.default_rng(7)
    return np.array([-1.0, 0.0, 2.0, 3.5, 9.0], F)[rng.integers(0, 5, 40)]


def overflow(L, seed=0):
    """exactly L distinct labels on 2 L rows, shuffled"""
    rng = np.random.default_rng(2000 + seed + L)
    lab = np.concatenate([distinct(L), distinct(L)])
    return lab[rng.permutation(len(lab))]


def all_different(M=20000):
    return np.random.default_rng(3).permutation(M).astype(F)


def values():
    """-> (labels, the distinct values in float order: -0.0 and +0.0 are one of them)"""
    one = np.nextafter(F(1.0), F(2.0))
    asc = np.array([-np.inf, -1e8, -3.25, -1.0, -1e-45, 0.0, 1e-45, 1.0, one, 2.5, 16777216.0, 3e38, np.inf], F)
    pool = np.concatenate([asc, asc, asc, np.array([-0.0, -0.0, 0.0, -0.0], F)])
    return pool[np.random.default_rng(11).permutation(len(pool))], asc


def zeros_only():
    """the issue's example: one cluster of four rows in original order between -1 and 1"""
    return np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], F)


def nans():
    """-> (labels, the bit patterns of the clusters in the table's order).  A signalling NaN of each sign (0x7f800001, 0xff800001:
    clusters of their own beside their quiet forms 0x7fc00001, 0xffc00001 -- an add in label_key would quiet them and merge the
    two), quiet NaNs of both signs with three payloads, the NaN of all ones and its neighbour 0x7ffffffe (one cluster, reported as
    the neighbour), the infinities and two finite labels."""
    pos = np.array([0x7F800001, 0x7FC00000, 0x7FC00001, 0x7FE12345, 0x7FFFFFFE, 0x7FFFFFFF], np.uint32)
    neg = np.array([0xFF800001, 0xFFC00000, 0xFFC00001, 0xFFE12345, 0xFFFFFFFF], np.uint32)
    fin = np.array([-np.inf, -2.0, 3.0, np.inf], F).view(np.uint32)
    pool = np.concatenate([pos, neg, fin, pos, neg, fin, pos[:2], neg[:1]])
    order = np.concatenate([neg[::-1], fin, pos[:5]])       # (the larger the bits of a negative NaN, the earlier)
    return pool[np.random.default_rng(13).permutation(len(pool))].view(F), order


def integer_pool(top):
    """the keys' home slots of the integer-valued labels 0 .. top - 1"""
    return tr.home_slot(tr.key(np.arange(top, dtype=F)))


@functools.lru_cache(maxsize=None)
def hash_labels(min_home):
    """the integer labels below 2^20 whose home slot is >= min_home, ascending"""
    return np.flatnonzero(integer_pool(1 << 20) >= min_home).astype(F)


@functools.lru_cache(maxsize=None)
def dense_labels(n):
    """n integer labels below 2^24 that share the home slot DENSE_HOME"""
    lab = np.flatnonzero(integer_pool(1 << 24) == DENSE_HOME).astype(F)
    return lab[:n]


def hash_cloud(labels, others=0, seed=0):
    """every label twice, mixed with `others` labels of their own (negative halves: no collision with the pool), shuffled"""
    rng = np.random.default_rng(4000 + seed)
    extra = -(np.arange(others, dtype=F) + 0.5)
    lab = np.concatenate([labels, labels, extra, extra[: others // 2]])
    return lab[rng.permutation(len(lab))]


def round_of_64(M=4096):
    """every aligned group of 64 rows holds the same 64 labels, each group in an order of its own"""
    rng = np.random.default_rng(5)
    v = distinct(64)
    return np.concatenate([v[rng.permutation(64)] for _ in range(M // 64)])


def giant(M=20000):
    """one label on 70 % of the rows, 500 labels on one row each, five labels on the rest"""
    rng = np.random.default_rng(6)
    big = np.full(M * 7 // 10, 7.0, F)
    single = 1000.0 + np.arange(500, dtype=F)
    rest = np.array([-1e8, -1.0, 1.0, 2.0, 3.0], F)[rng.integers(0, 5, M - len(big) - 500)]
    lab = np.concatenate([big, single, rest])
    return lab[rng.permutation(M)]


def once_per_chunk(n_chunks=5, L=300):
    """each of L labels exactly once in every 512-row chunk (the other 212 rows: -1), every chunk in an order of its own; a last
    chunk of L rows"""
    rng = np.random.default_rng(8)
    full = np.concatenate([distinct(L) + F(0.25), np.full(tr.CHUNK - L, -1.0, F)])
    return np.concatenate([full[rng.permutation(tr.CHUNK)] for _ in range(n_chunks)] + [(distinct(L) + F(0.25))[rng.permutation(L)]])


def pair_cases():
    """-> {name: (labelsA, labelsB, Lmax)}"""
    out = {}
    for ma, mb in PAIR_M:
        out[f"{ma} x {mb}"] = (seam_patterns(ma, 21)["seven iid"], seam_patterns(mb, 22)["sorted runs"], LMAX)
    out["1500 labels x 3"] = (counted(1500, 1), np.array([2.0, -1.0, 2.0, 5.0, -1.0], F), LMAX)
    out["3 x 1500 labels"] = (np.array([2.0, -1.0, 2.0, 5.0, -1.0], F), counted(1500, 1), LMAX)
    out["overflow x fits"] = (overflow(600), counted(100, 2), 512)
    out["fits x overflow"] = (counted(100, 2), overflow(600), 512)
    return out


def points_for(labels, seed=0):
    """any finite points: the order and the rows do not read them"""
    return np.random.default_rng(9000 + seed).uniform(-40, 40, (len(labels), 3)).astype(F)


def box(n, centre, extents, rng):
    """n float32 points in the box centre +- extents / 2; for n >= 2 the two opposite corners are among them"""
    c, h = np.asarray(centre, np.float64), np.asarray(extents, np.float64) / 2
    p = (c + rng.uniform(-1, 1, (n, 3)) * h).astype(F)
    p = np.clip(p, (c - h).astype(F), (c + h).astype(F))
    if n >= 2:
        p[0], p[-1] = (c - h).astype(F), (c + h).astype(F)
    return p


@functools.lru_cache(maxsize=None)
def stat_cloud(centre_name):
    """-> (points, labels): a cluster of every size of STAT_SIZES (labels 0, 1, ...; boxes of STAT_BOXES in turn) and 3000 rows of
    ground (-1e8) and noise (-1), rows shuffled"""
    rng = np.random.default_rng(sorted(STAT_CENTRES).index(centre_name) + 30)
    centre = np.asarray(STAT_CENTRES[centre_name])
    pts, lab = [], []
    for j, n in enumerate(STAT_SIZES):
        pts.append(box(n, centre + (j % 4) * 6.0, STAT_BOXES[j % len(STAT_BOXES)], rng))
        lab.append(np.full(n, float(j), F))
    pts.append(box(3000, centre, (80.0, 80.0, 3.0), rng))
    lab.append(np.where(rng.random(3000) < 0.7, -1e8, -1.0).astype(F))
    pts, lab = np.concatenate(pts), np.concatenate(lab)
    perm = rng.permutation(len(lab))
    return pts[perm], lab[perm]


@functools.lru_cache(maxsize=None)
def stat_one_cluster():
    rng = np.random.default_rng(41)
    return box(5000, STAT_CENTRES["3 km"], (4.5, 2.0, 1.0), rng)[rng.permutation(5000)], np.full(5000, 12.0, F)


@functools.lru_cache(maxsize=None)
def stat_many_clusters():
    """4096 clusters of 1 - 4 rows around (3000, -7000, 30), boxes of STAT_BOXES in turn"""
    rng = np.random.default_rng(42)
    lab = np.repeat(np.arange(4096, dtype=F), rng.integers(1, 5, 4096))
    pts = np.concatenate([box(int(n), np.asarray(STAT_CENTRES["3 km"]) + (j % 7), STAT_BOXES[j % len(STAT_BOXES)], rng)
                          for j, n in enumerate(np.bincount(lab.astype(np.int64)))])
    perm = rng.permutation(len(lab))
    return pts[perm], lab[perm]


def stat_cases():
    """-> {name: (points, labels)}"""
    out = {name: stat_cloud(name) for name in STAT_CENTRES}
    out["one cluster"] = stat_one_cluster()
    out["4096 clusters"] = stat_many_clusters()
    return out

"""Plain numpy restatement of the cluster table (csrc/table.hip: table_dict_kernel, table_count_kernel, table_scan_kernel,
table_scatter_kernel, table_stats_kernel) and of icpflow_cluster_stats (csrc/pose.hip), written from include/icpflow_hip.h:
the rows in a STABLE order by label, the distinct labels ascending with their counts and first positions, and per cluster the
centroid and the sorted bounding-box extents.  Shared by tests/test_table_restatement.py (CPU) and tests/test_gpu_tables.py.

The rules that are the library's own (the header states them):
  * -0.0 and +0.0 are one label, reported as 0.0;
  * NaN labels are one cluster per bit pattern, positive NaNs after +inf, negative NaNs before -inf (the order of the
    order-preserving map of the bits); the NaN of all ones shares a key with its neighbour 0x7ffffffe and is reported as that;
  * statistics for every label that is not < 0 (so for NaN labels too); six zeros for the others.
"""
import math
from fractions import Fraction

import numpy as np

F = np.float32
CHUNK = 512            # kChunkRows: rows of a chunk of the counting sort
DICT_ROUND = 8192      # rows table_dict_kernel takes per round
SLOTS = 8192           # kDictSlots
EMPTY = 0xFFFFFFFF     # kEmpty


def bits(labels):
    return np.ascontiguousarray(labels, dtype=F).view(np.uint32)


def key(labels):
    """float32 labels -> uint32 keys whose unsigned order is the table's order"""
    u = bits(labels).copy()
    u[(u & np.uint32(0x7FFFFFFF)) == 0] = 0                                  # both zeros: +0.0
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[k == np.uint32(EMPTY)] = np.uint32(EMPTY - 1)                          # the one NaN that collides with the empty mark
    return k


def label_of(k):
    """the float32 label a key is reported as"""
    k = np.asarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return u.view(F)


def quiet(label_bits):
    """the float32 bits a label reads back as from the table's float64 column: a signalling NaN comes back quiet (bit 22 set) --
    the conversions to float64 and back quiet it, on the device or on the host; every other pattern unchanged.  The CLUSTERS stay
    apart: a signalling NaN and its quiet form are two rows that read back as the same label."""
    b = np.asarray(label_bits, np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, b | np.uint32(0x00400000), b).astype(np.uint32)


def home_slot(k):
    """where table_dict_kernel's hash set first looks for a key: (key * 2654435761 mod 2^32) >> 19"""
    return ((np.asarray(k, np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)


def chunks(M):
    return (M + CHUNK - 1) // CHUNK


def table(labels):
    """-> order int64 [M], rows float64 [L, 3] = (label, count, start), label bits uint32 [L]"""
    k = key(labels)
    order = np.argsort(k, kind="stable").astype(np.int64)
    ks = k[order]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, np.int64)
    count = np.diff(np.concatenate([first, [len(ks)]]))
    lab = label_of(ks[first])
    with np.errstate(invalid="ignore"):          # (the conversion of a signalling NaN label raises the flag and quiets it)
        rows = np.stack([lab.astype(np.float64), count.astype(np.float64), first.astype(np.float64)], axis=1)
    return order, rows, bits(lab)


def stats(points, order, start, count, labels=None):
    """-> centroid float64 [L, 3] (math.fsum / n: the exactly rounded sum, one division), extents float32 [L, 3] ascending,
    mean |x| float64 [L, 3] (the scale of the summation bound).  labels given: clusters whose label is < 0 report zeros."""
    pts = np.asarray(points, F)
    L = len(start)
    mean, ext, mabs = np.zeros((L, 3)), np.zeros((L, 3), F), np.zeros((L, 3))
    for c in range(L):
        if labels is not None and labels[c] < 0:
            continue
        n = int(count[c])
        p = pts[order[int(start[c]):int(start[c]) + n]]
        for a in range(3):
            x = p[:, a].astype(np.float64)
            mean[c, a] = math.fsum(x) / n
            mabs[c, a] = math.fsum(np.abs(x)) / n
        ext[c] = np.sort(np.abs(p.max(axis=0) - p.min(axis=0)).astype(F))
    return mean, ext, mabs


def centroid_bound(m, n, mabs):
    """|got - m| allowed per axis: half a float32 step at |m| (the rounding of the result) + (n + 2) 2^-53 mean |x| -- n - 1
    additions in fp64 in any order (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order: each within
    2^-53 of a partial sum bounded by sum |x|), the division, and m's own two roundings.  Derived, not measured."""
    half = 0.5 * np.spacing(np.abs(np.asarray(m)).astype(F)).astype(np.float64)
    return half + (np.asarray(n, np.float64) + 2.0) * 2.0 ** -53 * np.asarray(mabs)


def exact_sum(x):
    """the sum of a float array as a Fraction: integers over one power of two, added by Python"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)
    mi = np.ldexp(m, 53).astype(np.int64)       # exact: 53-bit mantissas
    e = e.astype(np.int64) - 53
    lo = int(e.min())
    total = sum(int(a) << int(b) for a, b in zip(mi.tolist(), (e - lo).tolist()))
    return Fraction(total) * Fraction(2) ** lo

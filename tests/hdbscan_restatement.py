"""CPU restatements around the HDBSCAN spanning tree (csrc/hdbscan.hip) that reach beyond oracle/hdbscan.py's dense
matrices -- TEST INFRASTRUCTURE ONLY (tests/test_hdbscan_restatement.py pins them, tests/test_gpu_hdbscan_tree.py uses them).

oracle.hdbscan.mst holds several n x n fp64 matrices and stops near 4 000 rows: 64 chunks of 64 sorted rows, ONE group of
the kernels' chunk walk.  Everything here is NumPy / SciPy in fp64, squared distances as dx*dx + dy*dy + dz*dz left to right
(the oracle's and the kernels' order), under the kernels' strict total order on edges (w2, smaller caller row, larger caller
row), so that the tree is unique and compares edge for edge:

  prim_tree            Prim with O(n) memory: the tree of the complete graph, up to about 9 000 rows;
  tree_within_radius   the tree of the pairs within R, which CERTIFIES that it is the tree of the complete graph;
  sorted_layout        hdb_key_kernel's key, the stable sort, the chunks, their boxes and running x extremes;
  boruvka_on_tree      the kernels' rounds replayed on the finished tree: components, the giant that sits out;
  round0_proposals     the edge every row proposes in round 0.
The last three describe INPUTS (which seams, prunings and rounds a scene reaches), as cluster_shapes.hook_forest does for
DBSCAN; they are never compared with device state.
"""
from types import SimpleNamespace

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
from scipy.spatial import cKDTree

CELL_BITS = 21                         # cluster_util.hpp: kCellBits
MASKED_KEY = 0x7fffffffffffffff        # kMaskedKey: sorts after every real cell


def _xyz(points):
    P = np.ascontiguousarray(np.asarray(points)[:, :3], dtype=np.float64)
    return np.ascontiguousarray(P[:, 0]), np.ascontiguousarray(P[:, 1]), np.ascontiguousarray(P[:, 2])


def core2_blocked(points, k, block=512):
    """squared distance to the k-th nearest row, the row itself counted, in row blocks of `block` x n"""
    x, y, z = _xyz(points)
    out = np.empty(len(x))
    for s in range(0, len(x), block):
        dx, dy, dz = x[s:s + block, None] - x[None, :], y[s:s + block, None] - y[None, :], z[s:s + block, None] - z[None, :]
        out[s:s + block] = np.partition(dx * dx + dy * dy + dz * dz, k - 1, axis=1)[:, k - 1]
    return out


def _by_rows(a, b, w2):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    o = np.lexsort((hi, lo))
    return lo[o], hi[o], np.asarray(w2, np.float64)[o]


def prim_tree(points, k, ids=None):
    """-> (a, b, w2, core2) as oracle.hdbscan.mst: THE tree under (w2, smaller id, larger id), edges as rows a < b sorted
    by (a, b).  `ids` (a permutation; default the rows themselves) are what a tie is decided by.

    Prim from row 0 over the rows still outside: per step one row of squared distances, a lexicographic update of every
    outside row's best (weight, key) and a lexicographic arg-min.  The cut's lightest edge under a strict total order is
    a tree edge, and that tree is unique."""
    x, y, z = _xyz(points)
    n = len(x)
    c2 = core2_blocked(points, k)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    m = n - 1
    rem = np.arange(1, n)                                   # the outside rows; slots [0, m) are in use
    rx, ry, rz, rc, rid = x[1:].copy(), y[1:].copy(), z[1:].copy(), c2[1:].copy(), ids[1:].copy()
    bw = np.full(m, np.inf)
    bk = np.full(m, np.iinfo(np.int64).max)
    bfrom = np.full(m, -1, np.int64)
    ea, eb, ew = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m)
    v = 0
    for step in range(n - 1):
        dx, dy, dz = rx[:m] - x[v], ry[:m] - y[v], rz[:m] - z[v]
        w = np.maximum(np.maximum(rc[:m], c2[v]), dx * dx + dy * dy + dz * dz)
        idx = np.flatnonzero(w <= bw[:m])
        if len(idx):
            o = rid[idx]
            key = (np.minimum(o, ids[v]) << 32) | np.maximum(o, ids[v])
            idx2 = (w[idx] < bw[idx]) | (key < bk[idx])
            idx, key = idx[idx2], key[idx2]
            bw[idx], bk[idx], bfrom[idx] = w[idx], key, v
        cand = np.flatnonzero(bw[:m] == bw[:m].min())
        t = cand[np.argmin(bk[cand])]
        ea[step], eb[step], ew[step] = bfrom[t], rem[t], bw[t]
        v = rem[t]
        m -= 1                                              # the last slot in use moves into the freed one
        for arr in (rem, rx, ry, rz, rc, rid, bw, bk, bfrom):
            arr[t] = arr[m]
    return (*_by_rows(ea, eb, ew), c2)


def tree_within_radius(points, k, R):
    """-> (a, b, w2, core2) as prim_tree, from the pairs within R alone; raises ValueError unless the result is provably
    the tree of the COMPLETE graph:

      * every row has at least k - 1 pairs (so its k-th neighbour, itself counted, is among them: core2 is exact);
      * the pairs' minimum spanning forest has n - 1 edges (the pairs connect the cloud);
      * the heaviest tree weight is at most (0.99 R)^2.
    Then every omitted pair is farther than R (the KD-tree's own rounding is ~1e-16 relative, the margin 1 %), hence
    heavier than every edge on its tree path, hence no tree edge -- and no core distance exceeds the heaviest tree weight,
    because every row has a tree edge."""
    x, y, z = _xyz(points)
    n = len(x)
    P = np.stack([x, y, z], 1)
    pr = cKDTree(P).query_pairs(float(R), output_type="ndarray")
    i, j = np.minimum(pr[:, 0], pr[:, 1]).astype(np.int64), np.maximum(pr[:, 0], pr[:, 1]).astype(np.int64)
    dx, dy, dz = x[i] - x[j], y[i] - y[j], z[i] - z[j]
    d2 = dx * dx + dy * dy + dz * dz
    if k <= 1:
        c2 = np.zeros(n)
    else:
        rows, dd = np.concatenate([i, j]), np.concatenate([d2, d2])
        o = np.lexsort((dd, rows))
        rows, dd = rows[o], dd[o]
        cnt = np.bincount(rows, minlength=n)
        if cnt.min() < k - 1:
            raise ValueError(f"tree_within_radius: a row has {int(cnt.min())} pairs within R = {R}, {k - 1} are needed")
        c2 = dd[np.cumsum(cnt) - cnt + (k - 2)]
    w = np.maximum(np.maximum(c2[i], c2[j]), d2)
    order = np.lexsort((j, i, w))
    rank = np.empty(len(w))
    rank[order] = np.arange(1, len(w) + 1, dtype=np.float64)
    T = minimum_spanning_tree(coo_matrix((rank, (i, j)), shape=(n, n)).tocsr()).tocoo()
    if len(T.data) != n - 1:
        raise ValueError(f"tree_within_radius: the pairs within R = {R} leave {n - len(T.data)} components")
    e = order[np.rint(T.data).astype(np.int64) - 1]
    if n > 1 and w[e].max() > (0.99 * R) ** 2:
        raise ValueError(f"tree_within_radius: heaviest weight {np.sqrt(w[e].max())} is not inside 0.99 R = {0.99 * R}")
    return (*_by_rows(i[e], j[e], w[e]), c2)


def cell_coord(v, cell):
    """cluster_util.hpp cell_coord: floor((double)v * (1.0 / cell)) + 2^20, clamped to [1, 2^21 - 2] (finite v only)"""
    q = np.floor(np.asarray(v, np.float64) * (1.0 / float(cell))) + float(1 << (CELL_BITS - 1))
    return np.clip(q, 1.0, float((1 << CELL_BITS) - 2)).astype(np.int64)


def sorted_layout(points, mask=None, cell=0.25):
    """hdb_key_kernel + the stable radix sort + hdb_chunk_box_kernel + hdb_chunk_runs_kernel, restated.
    -> order (caller row at every sorted position), pos (its inverse), n_live, num_chunks = ceil(n / 64) over ALL rows,
    groups = ceil(num_chunks / 64), bmin / bmax [3, num_chunks] float32 (+inf / -inf for a chunk without live rows),
    suf_min_x / pre_max_x, chunk / group (of every caller row; -1 for rows that take no part)."""
    p = np.asarray(points)[:, :3].astype(np.float32)
    n = len(p)
    live = np.isfinite(p).all(1) & (np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool))
    q = np.where(live[:, None], p, 0.0)
    key = (cell_coord(q[:, 0], cell) << (2 * CELL_BITS)) | (cell_coord(q[:, 1], cell) << CELL_BITS) | cell_coord(q[:, 2], cell)
    key = np.where(live, key, MASKED_KEY)
    order = np.argsort(key, kind="stable")
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    n_live = int(live.sum())
    C = (n + 63) // 64
    pad = np.full((C * 64, 3), np.nan, np.float32)
    pad[:n_live] = p[order[:n_live]]
    pad = pad.reshape(C, 64, 3)
    with np.errstate(all="ignore"):
        bmin = np.where(np.isnan(pad), np.inf, pad).min(1).T.astype(np.float32)
        bmax = np.where(np.isnan(pad), -np.inf, pad).max(1).T.astype(np.float32)
    chunk = np.where(live, pos // 64, -1)
    return SimpleNamespace(order=order, pos=pos, live=live, n_live=n_live, num_chunks=C, groups=(C + 63) // 64, bmin=bmin, bmax=bmax,
                           suf_min_x=np.minimum.accumulate(bmin[0][::-1].astype(np.float64))[::-1],
                           pre_max_x=np.maximum.accumulate(bmax[0].astype(np.float64)), key=key,
                           chunk=chunk, group=np.where(live, chunk // 64, -1))


def _edge_rank(a, b, w2):
    """rank of every tree edge under (w2, smaller row, larger row)"""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    o = np.lexsort((hi, lo, w2))
    rank = np.empty(len(o), np.int64)
    rank[o] = np.arange(len(o))
    return rank, o


def round0_proposals(tree, n):
    """-> for every caller row that has a tree edge, the index (into the tree's arrays) of the edge it proposes in round
    0, -1 elsewhere.  A single row is a component, so its lightest edge to any other row is a tree edge (cut property):
    the lightest of its tree edges."""
    a, b, w2 = (np.asarray(t) for t in tree[:3])
    rank, o = _edge_rank(a, b, w2)
    best = np.full(n, len(a), np.int64)
    np.minimum.at(best, a, rank)
    np.minimum.at(best, b, rank)
    return np.where(best < len(a), o[np.minimum(best, len(a) - 1)], -1) if len(a) else np.full(n, -1, np.int64)


def boruvka_on_tree(tree, layout):
    """The kernels' rounds on the finished tree: every component's lightest outgoing edge is a tree edge, so the n - 1
    edges suffice.  A component is named by its smallest sorted position (uf_union hooks the larger root under the
    smaller); the giant of a round is the maximum of (size << 32 | root) over the components the round before produced
    (none in round 0) and sits the round out when its size exceeds 1.
    -> num_comp[r] and giant_size[r] (0 where no component sits out) for every round that still has > 1 component,
    closed by the final num_comp."""
    a, b, w2 = (np.asarray(t) for t in tree[:3])
    nl = layout.n_live
    pa, pb = layout.pos[a], layout.pos[b]                   # sorted positions of the edges' ends, all < n_live
    rank, o = _edge_rank(a, b, w2)
    comp = np.arange(nl)
    used = np.zeros(len(a), bool)
    num_comp, giant_size = [nl], []
    giant = 0
    while num_comp[-1] > 1:
        big = (giant & 0xffffffff) if (giant >> 32) > 1 else -1
        giant_size.append(int(giant >> 32) if big >= 0 else 0)
        ca, cb = comp[pa], comp[pb]
        cross = np.flatnonzero(ca != cb)
        assert len(cross) == num_comp[-1] - 1 and not used[cross].any()
        best = np.full(nl, len(a), np.int64)
        for c in (ca, cb):
            np.minimum.at(best, c[cross], rank[cross])
        if big >= 0:
            best[big] = len(a)
        pick = o[np.unique(best[best < len(a)])]
        used[pick] = True
        _, lab = connected_components(coo_matrix((np.ones(int(used.sum())), (pa[used], pb[used])), shape=(nl, nl)), directed=False)
        root = np.full(lab.max() + 1, nl, np.int64)
        np.minimum.at(root, lab, np.arange(nl))
        comp = root[lab]
        roots, sizes = np.unique(comp, return_counts=True)
        num_comp.append(len(roots))
        giant = int(((sizes.astype(np.int64) << 32) | roots).max())
    return SimpleNamespace(num_comp=num_comp, giant_size=giant_size)

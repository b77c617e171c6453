"""CPU: what tests/test_gpu_hdbscan_tree.py rests on.

  * tests/hdbscan_restatement.py is pinned: `prim_tree` to oracle.hdbscan.mst on the small cases of tests/test_cluster.py (all
    four arrays, bit for bit), `tree_within_radius` to `prim_tree` on 5 000 rows and to its own refusals, `sorted_layout` to
    the key's definition on hand-made rows, `boruvka_on_tree` to rounds replayed on the dense weight matrix;
  * every scene of tests/hdbscan_scenes.py keeps what it promises, in numbers: live rows, chunks and groups, the share of rows
    whose k-th neighbour / whose round-0 edge lies in another group, a probe round (r >= 3 with 1 < components <= n_live / 16)
    and a giant that sits out, and the scene's own condition.  The measured figures stand next to each bound.
No GPU, no library: a pass of the GPU module means what it claims only while these hold."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import hdbscan_restatement as hr
import hdbscan_scenes as hs
from conftest import load_golden
from oracle import hdbscan as oh
from test_cluster import _cloud, _lattice


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", ["lattice", "duplicates", "k1", "tiny", "crop_0"])
def test_prim_tree_equals_the_oracle(case):
    if case == "lattice":
        p, k = _lattice(14), 7
    elif case == "duplicates":
        p, k = np.repeat(_cloud(41, 300), 4, axis=0), 6
    elif case == "k1":
        p, k = _cloud(42, 1200), 1
    elif case == "tiny":
        p, k = _cloud(43, 9), 3
    else:
        g = load_golden("g11_hdbscan")
        p, k = g["crop_0_points"], int(g["crop_0_params"][0]) + 1
    want = oh.mst(p, k)
    assert same(hr.prim_tree(p, k), want)
    if case in ("lattice", "duplicates"):                      # dense enough for a radius; ties and zero distances
        assert same(hr.tree_within_radius(p, k, 6.0), want)


def test_prim_tree_ids_decide_ties_only():
    """with other ids the tree changes on a tied lattice and its weights do not; without ties (k = 1 on a random cloud) nothing changes"""
    p = _lattice(8)
    perm = np.random.default_rng(3).permutation(len(p))
    a, b = hr.prim_tree(p, 4), hr.prim_tree(p, 4, ids=perm)
    assert np.array_equal(np.sort(a[2]), np.sort(b[2])) and not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    # ids = the rows of the permuted cloud: the same tree as running on the permuted cloud, mapped back
    inv = np.argsort(perm)
    c = hr.prim_tree(p[inv], 4)                               # row r of the permuted cloud is row inv[r] here
    lo, hi = np.minimum(inv[c[0]], inv[c[1]]), np.maximum(inv[c[0]], inv[c[1]])
    o = np.lexsort((hi, lo))
    assert np.array_equal(lo[o], b[0]) and np.array_equal(hi[o], b[1]) and np.array_equal(c[2][o], b[2])
    q = _cloud(44, 400)                                       # k = 1: plain distances, all different (a core distance ties edges)
    assert len(np.unique(oh.sq_dists(q)[np.triu_indices(400, 1)])) == 400 * 399 // 2
    assert same(hr.prim_tree(q, 1, ids=np.random.default_rng(4).permutation(400)), hr.prim_tree(q, 1))


def test_tree_within_radius_equals_prim_tree_on_5000_rows():
    sc = hs.slab(5000, k=5)
    assert same(hr.tree_within_radius(sc.points, sc.k, 3.0), hr.prim_tree(sc.points, sc.k))


def test_tree_within_radius_refuses_what_it_cannot_certify():
    rng = np.random.default_rng(5)
    blob = rng.random((400, 3))                               # 400 rows in 1 m^3: neighbours at ~0.1 m
    with pytest.raises(ValueError, match="pairs within R"):
        hr.tree_within_radius(blob, 5, 0.05)                  # R too small for a 5-th neighbour
    two = np.concatenate([blob, blob + [10.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="components"):
        hr.tree_within_radius(two, 5, 1.0)                    # every row has its neighbours, the blobs never meet
    # joined by pairs between 0.99 R and R only: connected, yet an omitted pair could be as light
    a, b = np.array([[1.0, 0.5, 0.5]]), np.array([[3.0, 0.5, 0.5]])
    gap = np.concatenate([blob, a, blob + [3.0, 0.0, 0.0], b])
    with pytest.raises(ValueError, match="0.99 R"):
        hr.tree_within_radius(gap, 3, 2.0 / 0.995)
    assert same(hr.tree_within_radius(gap, 3, 2.5), hr.prim_tree(gap, 3))


def test_sorted_layout_on_rows_made_by_hand():
    p = np.array([[0.30, 0.0, 0.0],      # cell (1, 0, 0)
                  [-0.01, 0.0, 0.0],     # cell (-1, 0, 0): floor, not truncation
                  [0.0, 0.0, 0.0],       # cell (0, 0, 0)
                  [0.10, 0.0, -0.3],     # cell (0, 0, -2)
                  [np.nan, 0.0, 0.0],    # takes no part
                  [0.20, 0.0, 0.0],      # cell (0, 0, 0) again: stable, behind row 2
                  [0.0, np.inf, 0.0],    # takes no part
                  [-5.0, 0.0, 0.0]],     # masked
                 np.float32)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    lay = hr.sorted_layout(p, mask, 0.25)
    assert lay.order.tolist() == [1, 3, 2, 5, 0, 4, 6, 7] and lay.n_live == 5
    assert (lay.num_chunks, lay.groups) == (1, 1) and lay.group.tolist() == [0, 0, 0, 0, -1, 0, -1, -1]
    assert lay.bmin[:, 0].tolist() == [np.float32(-0.01), 0.0, np.float32(-0.3)] and lay.bmax[:, 0].tolist() == [np.float32(0.30), 0.0, 0.0]
    assert hr.cell_coord(np.float32(-0.25), 0.25) == (1 << 20) - 1 and hr.cell_coord(np.float32(-0.2500001), 0.25) == (1 << 20) - 2
    # the clamp: a cell of 1e-4 m leaves the 21-bit field beyond +-104 m, a cell of 1e5 m puts everything in cells -1 / 0
    assert hr.cell_coord([-200.0, 200.0], 1e-4).tolist() == [1, (1 << 21) - 2]
    assert hr.cell_coord([-200.0, 200.0], 1e5).tolist() == [(1 << 20) - 1, 1 << 20]
    # 130 rows, 70 of them dead: 3 chunks over ALL rows, the third without a live row
    q = np.zeros((130, 3), np.float32)
    q[:, 0] = np.arange(130)
    lay = hr.sorted_layout(q, np.arange(130) < 60, 0.25)
    assert (lay.n_live, lay.num_chunks) == (60, 3) and lay.bmin[0].tolist() == [0.0, np.inf, np.inf] and lay.bmax[0].tolist() == [59.0, -np.inf, -np.inf]
    assert lay.pre_max_x.tolist() == [59.0, 59.0, 59.0] and lay.suf_min_x.tolist() == [0.0, np.inf, np.inf]


def _dense_rounds(p, k, lay):
    """Boruvka's rounds on the dense weight matrix with the kernels' rules: -> (num_comp, giant_size) per round"""
    D2 = oh.sq_dists(p)
    c2 = np.partition(D2, k - 1, axis=1)[:, k - 1]
    W = np.maximum(np.maximum(c2[:, None], c2[None, :]), D2)
    n = len(p)
    comp = lay.pos.copy()                                     # component of every caller row = its smallest sorted position
    rows = np.arange(n)
    num_comp, giant_size, giant = [n], [], (0, -1)
    while num_comp[-1] > 1:
        big = giant[1] if giant[0] > 1 else -1
        giant_size.append(giant[0] if big >= 0 else 0)
        picks = []
        for c in np.unique(comp):
            if c == big:
                continue
            ins, out = rows[comp == c], rows[comp != c]
            w = W[np.ix_(ins, out)]
            ii, oo = np.nonzero(w == w.min())
            cand = sorted((min(ins[i], out[o]), max(ins[i], out[o])) for i, o in zip(ii, oo))
            picks.append(cand[0])
        for a, b in picks:
            ca, cb = comp[a], comp[b]
            if ca != cb:
                comp[comp == max(ca, cb)] = min(ca, cb)
        roots, sizes = np.unique(comp, return_counts=True)
        num_comp.append(len(roots))
        giant = max(zip(sizes.tolist(), roots.tolist()))
    return num_comp, giant_size


@pytest.mark.parametrize("case", ["cloud", "lattice", "duplicates"])
def test_boruvka_on_tree_equals_rounds_on_the_dense_matrix(case):
    p, k = {"cloud": (_cloud(45, 500), 4), "lattice": (_lattice(9)[np.random.default_rng(6).permutation(243)], 5),
            "duplicates": (np.repeat(_cloud(46, 120), 3, axis=0), 4)}[case]
    lay = hr.sorted_layout(p)
    b = hr.boruvka_on_tree(oh.mst(p, k), lay)
    want = _dense_rounds(p, k, lay)
    assert (b.num_comp, b.giant_size) == want
    assert len(b.giant_size) >= 2 and max(b.giant_size) > 1


def test_round0_proposals_are_every_rows_lightest_edge():
    p, k = _cloud(47, 300), 3
    a, b, w2, c2 = oh.mst(p, k)
    W = np.maximum(np.maximum(c2[:, None], c2[None, :]), oh.sq_dists(p))
    np.fill_diagonal(W, np.inf)
    prop = hr.round0_proposals((a, b, w2), len(p))
    for r in range(len(p)):
        near = np.flatnonzero(W[r] == W[r].min())
        other = min(near, key=lambda q: (min(r, q), max(r, q)))
        assert {int(a[prop[r]]), int(b[prop[r]])} == {r, int(other)}


# ------------------------------------------------------------------------------------------------ the scenes
def _facts(name):
    sc = hs.scene(name)
    lo, hi, w2, _ = hs.tree(name)
    lay = hr.sorted_layout(sc.points, sc.mask)
    rows = hs.live_rows(sc)
    assert lay.n_live == len(rows) and len(lo) == max(len(rows) - 1, 0)
    return sc, (lo, hi, w2), lay, rows


def _crossing_shares(sc, tree, lay, rows):
    """-> (rows whose k-th neighbour lies in another group, rows whose round-0 edge does), as counts"""
    lo, hi, _ = tree
    e = hr.round0_proposals(tree, len(sc.points))[rows]
    other = np.where(lo[e] == rows, hi[e], lo[e])
    P = sc.points[rows].astype(np.float64)
    _, ix = cKDTree(P).query(P, k=sc.k)
    kth = rows[ix[:, -1] if sc.k > 1 else ix]
    return int((lay.group[kth] != lay.group[rows]).sum()), int((lay.group[other] != lay.group[rows]).sum())


def _probe_rounds(b, n_live):
    """rounds in which hdb_scan_kernel's probe pass runs: r >= 3, more than one component, at most n_live >> 4"""
    return [r for r in range(3, len(b.giant_size)) if 1 < b.num_comp[r] <= (n_live >> 4)]


LAYOUT = {  # scene -> (rows, live rows, chunks, groups)
    "bar_x": (12300, 12300, 193, 4), "bar_y": (12300, 12300, 193, 4), "bar_z": (12300, 12300, 193, 4),
    "bridge": (9000, 9000, 141, 3), "bridge_mirrored": (9000, 9000, 141, 3), "twin_slabs": (8400, 8400, 132, 3),
    "equal_x": (8300, 8300, 130, 3), "folded_cell": (8320, 8320, 130, 3), "sparse_100": (9000, 100, 141, 3), "sparse_4097": (9000, 4097, 141, 3),
    "sparse_8193": (9000, 8193, 141, 3), "copies_70": (570, 570, 9, 1), "copies_63": (563, 563, 9, 1),
    "rows_64_k64": (64, 64, 1, 1), "rows_65_k64": (65, 65, 2, 1), "lattice_in_order": (4608, 4608, 72, 2),
    "lattice_shuffled": (4608, 4608, 72, 2), "wide_65600": (65600, 65600, 1025, 17),
}
LAYOUT.update({f"slab_{n}_{place}": (n, n, (n + 63) // 64, g) for n, g in hs.SEAM_SIZES.items() for place in hs.PLACES})
LAYOUT.update({f"cloud_{n}_k{k}": (n, n, (n + 63) // 64, 1 if n == 700 else 2) for n in (700, 4200) for k in (1, 2, 63, 64)})


def test_every_scene_is_listed():
    assert set(LAYOUT) == set(hs.SCENES)


@pytest.mark.parametrize("name", list(hs.SCENES))
def test_scene_layout_and_rounds(name):
    """rows, live rows, chunks, groups; the restated tree exists (tree_within_radius certified itself where it was used);
    on every scene of more than one group: a probe round whose bound prunes, and a giant that sits out"""
    sc, tree, lay, rows = _facts(name)
    assert (len(sc.points), lay.n_live, lay.num_chunks, lay.groups) == LAYOUT[name]
    assert sc.points.dtype == np.float32 and 1 <= sc.k <= 64
    b = hr.boruvka_on_tree(tree, lay)
    assert b.num_comp[-1] == 1 and len(b.giant_size) <= int(np.ceil(np.log2(max(lay.n_live, 2)))) + 1    # boruvka_rounds(n)
    print(f"{name}: components per round {b.num_comp}, giant sitting out {b.giant_size}, probe rounds {_probe_rounds(b, lay.n_live)}")
    if lay.groups > 1 and name != "lattice_in_order":          # (in meshgrid order the lattice is one component after two rounds)
        assert _probe_rounds(b, lay.n_live), b.num_comp
        assert max(b.giant_size) > 1


@pytest.mark.parametrize("place", list(hs.PLACES))
@pytest.mark.parametrize("n", list(hs.SEAM_SIZES))
def test_slab_searches_cross_the_group_seams(n, place):
    """Measured (origin / far / centred agree to a row or two): rows whose 5-th neighbour lies in another group 0, 1, 72,
    74, 161 of 4096, 4097, 8192, 8193, 8900; rows whose round-0 edge does 0, 1, 68, 56, 132.  At 4 097 rows the second
    group is ONE row (the largest cell key): it and nothing else crosses."""
    sc, tree, lay, rows = _facts(f"slab_{n}_{place}")
    kth, prop = _crossing_shares(sc, tree, lay, rows)
    print(f"slab {n} {place}: k-th neighbour in another group {kth} rows, round-0 edge {prop} rows")
    floor = {4096: 0, 4097: 1, 8192: 41, 8193: 41, 8900: 89}[n]          # 0.5 % and 1 % of the rows from two full groups on
    assert kth >= floor and prop >= floor
    assert (n > 4096) == (kth > 0)
    if place == "centred":
        assert (sc.points.min(0) < 0).all() and (sc.points.max(0) > 0).all()      # every coordinate straddles 0
    if place == "far":
        assert np.abs(sc.points[:, :2]).min() > 4000


@pytest.mark.parametrize("name", ["bar_x", "bar_y", "bar_z"])
def test_bars(name):
    sc, tree, lay, rows = _facts(name)
    axis = "xyz".index(name[-1])
    ext = sc.points.max(0) - sc.points.min(0)
    assert ext[axis] > 199 and (np.delete(ext, axis) < 1.0).all()
    xcells = np.unique(lay.key[rows] >> (2 * hr.CELL_BITS))
    if axis == 0:
        # the running extreme beyond a group away is farther than any tree weight: termination, not the box test, ends a walk
        assert len(xcells) > 790 and np.sqrt(tree[2].max()) < 1.0
    else:
        assert len(xcells) == 1 and ext[0] < 0.25                         # one x column: the x gap never exceeds the cell
        kth, prop = _crossing_shares(sc, tree, lay, rows)
        print(f"{name}: k-th neighbour in another group {kth} rows, round-0 edge {prop} rows")
        assert kth >= 20 and prop >= 12                                   # measured 24 / 15 (y), 2110 / 1740 (z)
    if axis == 2:
        # z is the LAST key field: a group is a y slab that spans all of z, so neighbours across a seam are everywhere
        assert _crossing_shares(sc, tree, lay, rows)[0] > 0.1 * len(rows)


@pytest.mark.parametrize("name", ["bridge", "bridge_mirrored"])
def test_bridge_edge_spans_the_chunk_table(name):
    sc, (lo, hi, w2), lay, rows = _facts(name)
    h = int(np.argmax(w2))
    far = np.sort(np.sqrt(w2))[-2:]
    assert far[1] > 140 and far[0] < 1.0                                   # ONE bridge
    ga, gb = sorted((int(lay.group[lo[h]]), int(lay.group[hi[h]])))
    print(f"{name}: the bridge joins sorted positions {lay.pos[lo[h]]} and {lay.pos[hi[h]]}")
    assert (ga, gb) == (0, 2)
    # the crescent's end of the bridge is not the crescent's row nearest in x: rows nearer in x are farther away
    arc = rows[np.abs(sc.points[rows, 0]) < 100]
    end = lo[h] if abs(sc.points[lo[h], 0]) < 100 else hi[h]
    behind = int((np.abs(sc.points[arc, 0]) > abs(sc.points[end, 0])).sum())
    print(f"{name}: {behind} of the crescent's {len(arc)} rows lie between the bridge's ends in x")
    assert len(arc) == 8700 and behind > 7800


def test_twin_slabs_interleave_through_every_chunk_column():
    sc, (lo, hi, w2), lay, rows = _facts("twin_slabs")
    far = np.sort(np.sqrt(w2))[-2:]
    assert far[1] > 139 and far[0] < 1.5
    upper = sc.points[lay.order[:lay.n_live], 1] > 100
    per_chunk = np.add.reduceat(upper.astype(int), np.arange(0, lay.n_live, 64))
    full = per_chunk[:lay.n_live // 64]
    assert (full > 0).all() and (full < 64).all()                          # both slabs in every full chunk
    assert np.array_equal(lay.bmin[1][:len(full)] < 20, lay.bmax[1][:len(full)] > 140)


def test_equal_x_runs_cross_the_chunk_and_group_borders():
    sc, tree, lay, rows = _facts("equal_x")
    xs = sc.points[lay.order[:lay.n_live], 0]
    borders = np.arange(64, lay.n_live, 64)
    inside = xs[borders - 1] == xs[borders]
    print(f"equal_x: {int(inside.sum())} of {len(borders)} chunk borders inside a run of equal x")
    assert inside.sum() >= 120 and inside[4096 // 64 - 1] and inside[8192 // 64 - 1]       # measured 124 of 129
    assert (np.unique(xs, return_counts=True)[1] == 100).all()
    assert np.array_equal(sc.points * 64, np.round(sc.points * 64))        # dyadic


def test_folded_cell_only_the_running_extremes_may_end_a_direction():
    """Measured: the 4-th neighbour of 3 785 of the 8 320 rows lies in another group; for 3 232 of them some chunk of the
    row's OWN group on that side has a box whose x gap alone exceeds the row's core distance -- a termination read from the
    chunk's own box would never reach that group -- and for none does the running extreme (which spans the cell)."""
    sc, tree, lay, rows = _facts("folded_cell")
    assert len(np.unique(lay.key)) == 1 and np.array_equal(lay.order, np.arange(len(sc.points)))
    c2 = hs.tree("folded_cell")[3]
    P = sc.points.astype(np.float64)
    _, ix = cKDTree(P).query(P, k=sc.k)
    kth, g, px = ix[:, -1], lay.group, P[:, 0]
    bmin, bmax = lay.bmin[0].astype(np.float64), lay.bmax[0].astype(np.float64)
    crossing = np.flatnonzero(g[kth] != g)
    own_box = running = 0
    for r in crossing:
        if g[kth[r]] > g[r]:
            ts = np.arange(lay.chunk[r] + 1, min((g[r] + 1) * 64, lay.num_chunks))
            d, dr = bmin[ts] - px[r], lay.suf_min_x[ts] - px[r]
        else:
            ts = np.arange(g[r] * 64, lay.chunk[r])
            d, dr = px[r] - bmax[ts], px[r] - lay.pre_max_x[ts]
        own_box += bool(((d > 0) & (d * d > c2[r])).any())
        running += bool(((dr > 0) & (dr * dr > c2[r])).any())
    print(f"folded_cell: k-th neighbour in another group {len(crossing)} rows; own-box termination would cut {own_box} of them off, the running extreme {running}")
    assert len(crossing) >= 3000 and own_box >= 2500 and running == 0


@pytest.mark.parametrize("n_live", [100, 4097, 8193])
def test_sparse_scenes_interleave_dead_rows_of_every_kind(n_live):
    sc, tree, lay, rows = _facts(f"sparse_{n_live}")
    fin = np.isfinite(sc.points).all(1)
    assert (~sc.mask).sum() > 0 and (sc.mask & ~fin).sum() > 0 and (~sc.mask & ~fin).sum() == 0
    assert np.isnan(sc.points).any() and (sc.points == np.inf).any() and (sc.points == -np.inf).any()
    assert n_live % 64 not in (0,) and np.diff(rows).max() > 1 and rows[0] < 200 and rows[-1] > 8800       # interleaved
    last = (n_live - 1) // 64
    assert np.isfinite(lay.bmin[:, :last + 1]).all() and (lay.bmin[:, last + 1:] == np.inf).all() and (lay.bmax[:, last + 1:] == -np.inf).all()
    assert lay.num_chunks - last - 1 >= 12                                  # all-dead chunks behind the live ones


@pytest.mark.parametrize("m", [70, 63])
def test_copies_core_distance(m):
    sc, tree, lay, rows = _facts(f"copies_{m}")
    c2 = hs.tree(f"copies_{m}")[3]
    dup = np.flatnonzero((sc.points == sc.points[np.argmax((sc.points[:, None, 0] == sc.points[None, :, 0]).sum(1))]).all(1))
    assert len(dup) == m
    assert (c2[dup] == 0).all() if m >= 64 else (c2[dup] > 0).all()
    assert (np.delete(c2, dup) > 0).all()


def test_shuffled_lattice_ties_are_decided_by_caller_rows():
    """Every weight of the lattice's tree is tied.  Measured: ranking the tree's edges by (w2, rows) and by (w2, sorted
    positions) disagrees on 4 607 of 4 607 edges of the shuffled copy (none in meshgrid order), and Prim with positions as
    ids yields a tree that differs in 3 277 edges."""
    sc, (lo, hi, w2), lay, rows = _facts("lattice_shuffled")
    assert (np.unique(w2, return_counts=True)[1] > 1).all()
    plo, phi = np.minimum(lay.pos[lo], lay.pos[hi]), np.maximum(lay.pos[lo], lay.pos[hi])
    disagree = int((np.lexsort((hi, lo, w2)) != np.lexsort((phi, plo, w2))).sum())
    other = hr.prim_tree(sc.points, sc.k, ids=lay.pos)
    mine = set(zip(lo.tolist(), hi.tolist()))
    differ = len(mine - set(zip(other[0].tolist(), other[1].tolist())))
    print(f"shuffled lattice: ranks disagree on {disagree} of {len(lo)} tied edges; the tree keyed on positions differs in {differ} edges")
    assert disagree * 3 >= len(lo) and differ >= 100
    assert np.array_equal(np.sort(other[2]), np.sort(w2))
    # in meshgrid order rows and positions are one order: that copy cannot tell the two rules apart
    ordered = hs.scene("lattice_in_order")
    assert np.array_equal(hr.sorted_layout(ordered.points).pos, np.arange(len(ordered.points)))


def test_wide_scene_takes_two_chunks_per_scan_thread():
    sc, tree, lay, rows = _facts("wide_65600")
    per = (lay.num_chunks + 1023) // 1024
    assert per == 2 and (lay.num_chunks + per - 1) // per == 513          # threads 513 ... 1023 hold no chunk
    assert 65537 <= lay.n_live <= 65600
    # the running extremes change along the table (a scan that dropped a carry would show): many distinct values
    assert len(np.unique(lay.pre_max_x)) > 60 and len(np.unique(lay.suf_min_x)) > 60

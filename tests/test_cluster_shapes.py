"""CPU: conditions on the inputs of tests/test_gpu_cluster_shapes.py (tests/cluster_shapes.py), so that a GPU pass means
something: the two statements of DBSCAN agree on every shape, the thin shapes really merge hundreds of hook trees into one
cluster, `walls` really has contested border points, `exact_pairs` really sits at eps exactly and reaches all 26 neighbour
cells.  The counted figures are printed (pytest -s), so a change of a generator shows in the log."""
import numpy as np
import pytest

import cluster_shapes as cs
from oracle import cluster as oc
from test_cluster import _cloud

EPS = 0.25

THIN = {
    "comb": lambda **kw: cs.comb(**kw),
    "spiral": lambda **kw: cs.spiral(6000, **kw),
    "snake": lambda **kw: cs.snake(**kw),
}


@pytest.mark.parametrize("seed,n,eps,mp,want", [(13, 257, 0.3, 4, (11, 19, 3, 1)), (14, 5000, 0.2, 6, (10, 68, 10, 0)),
                                                (16, 3000, 0.05, 3, (73, 76, 2, 0)), (17, 3000, 3.0, 40, (1, 6, 6, 0)),
                                                (18, 4096, 0.25, 1, (831, 906, 14, 0))])
def test_hook_forest_counts_on_the_blobs_the_suite_already_had(seed, n, eps, mp, want):
    """The instrument on tests/test_cluster.py's Gaussian blobs: (clusters, hook trees, most trees in one cluster, contested
    border points), counted once and pinned -- a few trees per cluster, one contested point in all of them."""
    f = cs.hook_forest(_cloud(seed, n), eps, mp)
    got = (f.clusters, f.trees, f.max_trees_in_cluster, f.contested)
    print(f"_cloud({seed}, {n}) eps {eps} mp {mp}: clusters, trees, max trees in one cluster, contested = {got}")
    assert got == want
    assert f.clusters == int(oc.dbscan_components(_cloud(seed, n), eps, mp).max()) + 1


@pytest.mark.parametrize("name", ["comb", "spiral", "snake"])
def test_thin_shapes_are_one_cluster_of_at_least_100_hook_trees(name):
    for mp in (2, 3):
        p = THIN[name]()
        lab = oc.dbscan_components(p, EPS, mp)
        assert (lab == 0).all()
        assert np.array_equal(oc.dbscan_index_order(p, EPS, mp), lab)
    for shuffle in (None, 1):
        p = THIN[name](shuffle=shuffle)
        f = cs.hook_forest(p, EPS, 2)
        print(f"{name} ({len(p)} points, shuffle {shuffle}): {f.trees} hook trees in {f.clusters} cluster")
        assert f.clusters == 1 and f.contested == 0
        # rows in order along x: the stable sort keeps them so and most points hook to the one before (comb 48, snake 18
        # trees); the spiral crosses cells in every direction and needs no shuffle
        assert f.max_trees_in_cluster == f.trees >= (100 if shuffle is not None or name == "spiral" else 1)
    for offset in ("centre", cs.FAR):                      # the placements of the GPU test keep it one cluster
        assert (oc.dbscan_components(THIN[name](shuffle=1, offset=offset), EPS, 2) == 0).all()


def test_generators_have_the_stated_sizes():
    assert len(cs.comb()) == 3022 and len(cs.snake()) == 1558 and len(cs.spiral(6000)) == 6000
    assert len(cs.walls()) == 6 * cs.WALL_ROWS + 5 and len(cs.dust(40)) == 3200
    for g in (cs.comb(), cs.snake(), cs.spiral(100), cs.walls(), cs.dust(3), cs.dashes(7)):
        assert g.dtype == np.float32 and g.shape[1] == 3
    a, b = cs.comb(shuffle=3), cs.comb()
    assert not np.array_equal(a, b) and np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
    d = np.linalg.norm(np.diff(cs.spiral(3000).astype(np.float64), axis=0), axis=1)     # chords of a 0.2 arc
    assert d.max() <= 0.2 + 1e-6 and d[50:].min() > 0.199


def test_comb_without_its_spine_is_48_clusters():
    p, spine = cs.comb(shuffle=2, parts=True)
    assert spine.sum() == 142
    lab = oc.dbscan_components(p[~spine], EPS, 2)
    assert lab.max() + 1 == 48 and (np.bincount(lab) == 60).all()
    assert np.array_equal(oc.dbscan_index_order(p[~spine], EPS, 2), lab)


def test_walls_have_five_contested_points_that_want_the_lower_id():
    p = cs.walls()
    lab = oc.dbscan_components(p, EPS, 8)
    assert np.array_equal(oc.dbscan_index_order(p, EPS, 8), lab)
    f = cs.hook_forest(p, EPS, 8)
    print(f"walls: {f.clusters} clusters, {f.trees} hook trees, {f.contested} contested points, labels {lab[-5:]}")
    assert f.clusters == 6 and f.contested == 5
    lone = np.arange(6 * cs.WALL_ROWS, len(p))
    assert np.array_equal(f.contested_rows, lone) and not f.core[lone].any()
    pairs = oc.radius_pairs(p, EPS)
    for c, row in enumerate(lone):
        nb = np.r_[pairs[pairs[:, 0] == row, 1], pairs[pairs[:, 1] == row, 0]]
        assert len(nb) == 6 and f.core[nb].all()
        ids = np.unique(lab[nb])
        assert np.array_equal(ids, [4 - c, 5 - c])                 # its two walls; the sort order meets 5 - c first
        assert lab[row] == ids.min()
    assert np.array_equal(lab[lone], [4, 3, 2, 1, 0])
    # the walls' ends: three rows at each end are no core points and belong to their own wall alone
    for w in range(6):
        rows = np.arange(w * cs.WALL_ROWS, (w + 1) * cs.WALL_ROWS)
        assert (lab[rows] == w).all()
        assert not f.core[rows[[0, 1, 2, -3, -2, -1]]].any() and f.core[rows[3:-3]].all()
    # the keys run against the ids: wall 0 (cluster 5) sorts first
    k = cs.keys(p, EPS)
    assert all(k[(5 - c) * cs.WALL_ROWS:(6 - c) * cs.WALL_ROWS].max() < k[(4 - c) * cs.WALL_ROWS:(5 - c) * cs.WALL_ROWS].min() for c in range(5))


@pytest.mark.parametrize("n", [1, 5, 64, 257, 8193])
def test_dashes_are_runs_of_fifty(n):
    p = cs.dashes(n)
    lab = oc.dbscan_components(p, EPS, 1)
    sizes = np.bincount(lab)
    assert len(sizes) == -(-n // 50)
    assert sorted(sizes.tolist()) == sorted([50] * (n // 50) + ([n % 50] if n % 50 else []))
    if n <= 257:
        assert np.array_equal(oc.dbscan_index_order(p, EPS, 1), lab)
        assert np.array_equal(oc.dbscan_index_order(p, EPS, 2), oc.dbscan_components(p, EPS, 2))


def test_dust_is_one_cluster_per_point():
    p = cs.dust(12)
    assert np.array_equal(oc.dbscan_components(p, EPS, 1), np.arange(len(p)))
    assert np.array_equal(oc.dbscan_index_order(p, EPS, 1), np.arange(len(p)))


def test_exact_pairs_sit_at_eps_exactly_and_reach_all_26_neighbour_cells():
    from scipy.spatial import cKDTree
    sets = cs.exact_pairs()
    assert [e for e, _ in sets] == [7 / 32, 3 / 8]
    for (eps, p), n_pairs in zip(sets, (48 * 7, 24 * 7)):
        assert p.dtype == np.float32 and len(p) == 2 * n_pairs
        q = p.astype(np.float64)
        d = q[0::2] - q[1::2]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        assert (d2 == eps * eps).all()                               # exactly: not below, so no neighbours
        assert (d2 < np.nextafter(eps, 1) ** 2).all()
        assert len(np.unique(d, axis=0)) == (48 if eps < 0.25 else 24)      # every permutation and sign pattern
        near = cKDTree(q).query_pairs(1.0, output_type="ndarray")
        assert np.array_equal(near[np.argsort(near[:, 0])], np.arange(2 * n_pairs).reshape(-1, 2))   # the pairs, nothing else
        c = cs.cells(p, eps)
        offsets = {tuple(o) for o in (c[1::2] - c[0::2]).tolist()}
        want = {(a, b, e) for a in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)} - {(0, 0, 0)}
        assert offsets == want
        bias = 1 << 20
        assert (c[:, 0] < bias).any() and (c[:, 0] > bias).any() and (c[:, 1:] < bias).any() and (c[:, 1:] > bias).any()
        assert ((p == 0) & ~np.signbit(p)).any() and ((p == 0) & np.signbit(p)).any()     # 0.0 and -0.0
        print(f"exact_pairs eps {eps}: {n_pairs} pairs, {len(offsets)} cell offsets")
        assert (oc.dbscan_components(p, eps, 2) == -1).all()
        assert np.array_equal(oc.dbscan_components(p, np.nextafter(eps, 1), 2), np.arange(2 * n_pairs) // 2)
        assert np.array_equal(oc.dbscan_index_order(p, np.nextafter(eps, 1), 2), np.arange(2 * n_pairs) // 2)

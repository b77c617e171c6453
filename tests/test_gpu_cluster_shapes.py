"""GPU: DBSCAN (icpflow_dbscan, icpflow_cluster_pcd; csrc/cluster.hip) and the HDBSCAN spanning tree on THIN shapes.

A Gaussian blob is a handful of hook trees per cluster; a comb, a spiral or a snake (tests/cluster_shapes.py) is one cluster
of hundreds, so nearly every point's component is decided by the lock-free unions and by the roots published behind them.
`walls` makes five border points choose between two clusters whose ids run against the sort order; `dashes` puts the row count
on every block, chunk and slice border of the kernels; `exact_pairs` sits at distance eps exactly in all 26 neighbour cells.
Labels and sizes are compared with `np.array_equal` against oracle.cluster.dbscan_components: labels are indices, there is no
tolerance.  The conditions on the inputs themselves are tests/test_cluster_shapes.py (CPU)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import cluster_shapes as cs  # noqa: E402
from icp_flow_amd import utils_cluster  # noqa: E402
from oracle import cluster as oc, hdbscan as oh  # noqa: E402
from test_cluster import _gpu_tree  # noqa: E402
from test_gpu_cluster_pcd import G, _args, both_paths  # noqa: E402

EPS = 0.25
SHAPES = {
    "comb": lambda **kw: cs.comb(**kw),
    "spiral": lambda **kw: cs.spiral(6000, **kw),
    "snake": lambda **kw: cs.snake(**kw),
}
PLACES = {"origin": None, "centred": "centre", "far": cs.FAR}


def check(p, eps, mp, mask=None):
    """labels and sizes of icpflow_dbscan against the oracle on the live rows (-2 on masked ones); -> the wanted labels"""
    lab, sizes = utils_cluster.dbscan(p, eps, mp, mask)
    sel = np.ones(len(p), bool) if mask is None else np.asarray(mask, bool)
    want = np.full(len(p), -2, np.int64)
    fin = sel & np.isfinite(p).all(1)
    want[sel] = -1
    want[fin] = oc.dbscan_components(p[fin], eps, mp)
    got = lab.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (int((got != want).sum()), len(p))
    c = int(want.max()) + 1
    assert sizes.numel() == c
    assert np.array_equal(sizes.cpu().numpy(), np.bincount(want[want >= 0], minlength=c))
    return want


@pytest.mark.parametrize("mp", [2, 3])
@pytest.mark.parametrize("place", list(PLACES))
@pytest.mark.parametrize("shuffle", [None, 1], ids=["in_order", "shuffled"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_thin_shapes_are_one_cluster(name, shuffle, place, mp):
    want = check(SHAPES[name](shuffle=shuffle, offset=PLACES[place]), EPS, mp)
    assert (want == 0).all()


def test_comb_with_its_spine_masked_or_not_finite_is_48_clusters():
    p, spine = cs.comb(shuffle=2, parts=True)
    want = check(p, EPS, 2, ~spine)                       # masked rows report -2 and bridge nothing
    assert (want[spine] == -2).all() and want.max() + 1 == 48 and (np.bincount(want[~spine]) == 60).all()
    bad = p.copy()
    bad[spine, 1] = np.nan                                # not finite: never cluster, never join, report -1
    want = check(bad, EPS, 2)
    assert (want[spine] == -1).all() and want.max() + 1 == 48 and (np.bincount(want[~spine]) == 60).all()


@pytest.mark.parametrize("shuffle", [None, 5], ids=["ids_against_sort_order", "shuffled"])
def test_walls_contested_points_take_the_lower_id(shuffle):
    p = cs.walls(shuffle=shuffle)
    want = check(p, EPS, 8)
    assert want.max() + 1 == 6
    if shuffle is None:
        lab = utils_cluster.dbscan(p, EPS, 8)[0].cpu().numpy()
        assert np.array_equal(lab[-5:], [4, 3, 2, 1, 0])            # each between clusters (4 - c, 5 - c): the minimum
        for w in range(6):                                          # the walls' ends: plain border points of their wall
            assert (lab[w * cs.WALL_ROWS:(w + 1) * cs.WALL_ROWS] == w).all()


def test_dust_is_as_many_clusters_as_points():
    p = cs.dust(40)
    lab, sizes = utils_cluster.dbscan(p, EPS, 1)
    assert sizes.numel() == len(p) == 3200 and bool((sizes == 1).all())
    assert np.array_equal(lab.cpu().numpy(), np.arange(len(p)))
    check(cs.dust(40, shuffle=3, offset="centre"), EPS, 1)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 8191, 8192, 8193])
def test_dashes_at_the_kernels_edges(n):
    """n around 4 points per workgroup (the wave-per-point kernels), the 64-row chunks of chunkRoot, the 256-thread blocks and
    the 512-row slices of the rank kernel's sixteen waves (1024 rows from 8193 on)."""
    p = cs.dashes(n)
    want = check(p, EPS, 1)
    assert want.max() + 1 == -(-n // 50)
    assert sorted(np.bincount(want).tolist()) == sorted([50] * (n // 50) + ([n % 50] if n % 50 else []))
    check(p, EPS, 2)                                       # a run of one point is noise now, the runs' ends are core points
    check(p, EPS, 3)                                       # ... and border points now


@pytest.mark.parametrize("split", ["one_cell", "two_x_cells", "two_z_cells"])
def test_core_count_across_ballots_and_runs(split):
    """130 copies of a point: three ballots of 64 candidates.  A cluster at min_points 130, noise at 131 -- also when the copies
    sit 1 mm apart on both sides of a cell border (two runs of the 9, resp. one run over two cells)."""
    p = np.tile(np.array([[1.0, -2.0, 0.5]], np.float32), (130, 1))
    if split != "one_cell":
        ax = 0 if split == "two_x_cells" else 2
        p[:, ax] = 0.0
        p[::2, ax] = -1e-3
        c = cs.cells(p, 0.1)[:, ax]
        assert set(np.unique(c)) == {(1 << 20) - 1, 1 << 20}
    assert (check(p, 0.1, 130) == 0).all()
    assert (check(p, 0.1, 131) == -1).all()
    assert (check(p, 0.1, 129) == 0).all()


@pytest.mark.parametrize("k", [0, 1], ids=["7/32", "3/8"])
def test_exact_pairs_are_noise_at_eps_and_clusters_just_above(k):
    eps, p = cs.exact_pairs()[k]
    assert (check(p, eps, 2) == -1).all()
    assert np.array_equal(check(p, float(np.nextafter(eps, 1)), 2), np.arange(len(p)) // 2)
    assert (check(p, float(np.nextafter(eps, 0)), 2) == -1).all()


def test_labels_are_a_function_of_the_input():
    p = G(cs.spiral(6000, shuffle=1))
    runs = [utils_cluster.dbscan(p, EPS, 2) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        runs.append(utils_cluster.dbscan(p, EPS, 2))
    side.synchronize()
    for lab, sizes in runs:
        assert torch.equal(lab, runs[0][0]) and torch.equal(sizes, runs[0][1])
    assert bool((runs[0][0] == 0).all()) and runs[0][1].tolist() == [6000]


@pytest.mark.parametrize("mp,clusters", [(2, 48 + 3), (8, 6)])
def test_cluster_pcd_native_on_comb_and_walls_equals_the_numpy_path(mp, clusters):
    """dst = the comb without its spine (mask), src = the walls 10 m aside without two of the lone points (mask): at
    min_points 2 the remaining lone points join their walls in pairs, at 8 the comb is noise and the walls are six."""
    comb, spine = cs.comb(shuffle=4, parts=True)
    wall = cs.walls(offset=(0.0, -10.0, 0.0))
    p = np.concatenate([comb, wall])
    keep_src = np.ones(len(wall), bool)
    keep_src[[-4, -2]] = False
    mask = np.concatenate([~spine, keep_src])
    a = _args(EPS, mp, 200)                                  # every cluster is kept: no tie in size at the cut
    got = both_paths(a, G(p), G(mask), n_dst=len(comb)).cpu().numpy()
    assert np.array_equal(got, oc.cluster_pcd(a, p, mask))
    raw = oc.dbscan_components(p[mask], EPS, mp)
    assert raw.max() + 1 == clusters


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("name", ["comb", "snake", "spiral"])
def test_spanning_tree_of_thin_shapes_equals_oracle_edge_for_edge(name, k):
    """The scheme of test_cluster.test_gpu_spanning_tree_equals_oracle_edge_for_edge.  On the comb one weight makes up most of
    the tree, so the tie rule decides nearly every edge; the spiral gives Boruvka many rounds of chained unions."""
    p = {"comb": lambda: cs.comb(shuffle=1), "snake": lambda: cs.snake(shuffle=1), "spiral": lambda: cs.spiral(3000, shuffle=1)}[name]()
    lo, hi, w2, c2, n_live = _gpu_tree(p, k)
    ra, rb, rw, rc = oh.mst(p, k)
    if name == "comb":
        assert np.unique(rw, return_counts=True)[1].max() >= 1000
    assert n_live == len(p) and len(lo) == len(p) - 1
    assert np.array_equal(c2, rc)
    assert np.array_equal(lo, ra) and np.array_equal(hi, rb) and np.array_equal(w2, rw)

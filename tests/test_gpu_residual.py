"""icpflow_nn_residual on the GPU against the numpy restatement (tests/residual_restatement.py, itself checked against exact
integer arithmetic in tests/test_residual.py): d2 and idx bit for bit, the table's counts equal, its sums within
(rows - 1) 2^-53 sum of math.fsum, every output between guards on a poisoned workspace of exactly the size the library asks for
(tests/residual_device.py).  Shapes over the wave, workgroup and scan-tile edges; geometry that breaks a grid search (ties,
d2 == r2, cell borders, far coordinates, one crowded cell, colliding buckets); bad rows and every optional argument; reruns and
streams; the dyadic clouds against the integer statement directly; and a frame pair end to end through run_stream."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd             # noqa: E402
import residual_restatement as rr        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = rd.DEV
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2049)
EDGES = (0.05, 0.1)


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_shapes_over_the_wave_block_and_scan_tile_edges(n):
    """m = 511, 512, 513 give H = 1024, 1024, 2048 buckets: one scan tile, one full, two; 2049 gives five"""
    hits = 0
    for k, m in enumerate(SIZES):
        q, t, f, g = rd.scene(n, m, seed=1000 * n + m, span=4.0, radius=1.0, G=3)
        got, _ = rd.check(q, t, f, 1.0, g, 3, EDGES, label=f"{n} x {m}", poison=(0x00, 0xA5, 0xFF)[k % 3])
        hits += int((got["idx"] >= 0).sum())
    assert hits > 0 or n == 0


def test_twenty_thousand_by_twenty_thousand():
    q, t, f, g = rd.scene(20000, 20000, seed=7, span=40.0, radius=2.0, G=4)
    got, _ = rd.check(q, t, f, 2.0, g, 4, EDGES, label="20000 x 20000")
    assert 0.3 < float((got["idx"] >= 0).mean()) < 1.0
    assert int(got["info"][2]) > 1000 and int(got["info"][3]) >= 1        # occupied buckets, the longest bucket


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_duplicated_targets_and_lattices_go_to_the_lowest_row():
    rng = np.random.default_rng(3)
    ax = np.arange(-5, 5) * 0.5
    lattice = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    t = np.concatenate([lattice, lattice[rng.integers(0, 1000, 300)]])[rng.permutation(1300)].astype(np.float32)
    on = lattice[rng.integers(0, 1000, 200)]
    q = np.concatenate([on, on + rng.choice([0.0, 0.25], (200, 3)), on + 0.25]).astype(np.float32)     # on, between, at cell centres
    for radius in (0.25, 0.5, 1.0):
        got, (d2, idx, _, _) = rd.check(q, t, None, radius, label=f"lattice r {radius}")
        # the rule itself, not only the restatement's word for it: no lower row is as near
        D = ((q[:, None, :].astype(np.float64) - t[None, :, :]) ** 2).sum(axis=2)
        ties = 0
        for i in np.flatnonzero(got["idx"] >= 0):
            same = np.flatnonzero(D[i] == D[i].min())
            assert got["idx"][i] == same[0]
            ties += len(same) > 1
        assert ties > 100


def test_d2_equal_to_r2_is_a_hit_and_the_next_float_is_a_miss():
    f32 = np.float32
    for radius in (1.0, 0.3, 2.0, 1e-3, 777.7):
        r = f32(radius)
        r2 = r * r
        t = np.zeros((1, 3), np.float32)
        q = np.array([[r, 0, 0], [np.nextafter(r, f32(np.inf)), 0, 0], [0, -r, 0], [0, 0, np.nextafter(r, f32(0))]], np.float32)
        got, _ = rd.check(q, t, None, radius, label=f"r {radius}")
        assert got["idx"].tolist() == [0, -1, 0, 0] and got["d2"][0] == r2 and got["d2"][1] == r2 and got["d2"][3] < r2


def test_queries_on_cell_borders_and_at_negative_coordinates():
    """cell edge h = 1.01 r: queries and targets a few float32 steps either side of multiples of h, both signs"""
    rng = np.random.default_rng(4)
    for radius in (1.0, 0.37):
        h = 1.01 * radius
        k = rng.integers(-6, 7, (600, 3))
        q = (k * h).astype(np.float32)
        for _ in range(3):
            step = rng.integers(-2, 3, q.shape)
            q = np.where(step > 0, np.nextafter(q, np.float32(np.inf)), np.where(step < 0, np.nextafter(q, np.float32(-np.inf)), q)).astype(np.float32)
        t = (q[rng.integers(0, 600, 900)].astype(np.float64) + rng.choice([-1.0, 0.0, 1.0], (900, 3)) * radius *
             rng.choice([1.0, 0.999999, 0.5], (900, 1))).astype(np.float32)
        got, _ = rd.check(q, t, None, radius, label=f"borders r {radius}")
        assert 0.2 < float((got["idx"] >= 0).mean())


def test_far_scenes():
    """a scene 3 km out; a scene at +-(1e6 - 1) m with r = 1e-3, where float32 steps by 1/16 m: only coincident points are
    neighbours, exactly 1e6 is still a good row and the row beyond it is bad"""
    q, t, f, g = rd.scene(700, 900, seed=9, span=10.0, radius=0.5, centre=(3000.0, -3000.0, 50.0), G=2)
    got, _ = rd.check(q, t, f, 0.5, g, 2, EDGES, label="3 km")
    assert 0.2 < float((got["idx"] >= 0).mean()) < 1.0
    rng = np.random.default_rng(10)
    corner = np.array([999999.0, -999999.0, 999999.0])
    t = (corner + rng.integers(-8, 9, (400, 3)) / 16.0 * np.sign(-corner)).astype(np.float32)
    t = np.concatenate([t, np.array([[1e6, -1e6, 1e6], [1000001.0, 0, 0], [0, -1000001.0, 0]], np.float32)])
    q = np.concatenate([t[rng.integers(0, 400, 200)], (corner + rng.integers(-8, 9, (200, 3)) / 16.0 * np.sign(-corner)).astype(np.float32),
                        np.array([[1e6, -1e6, 1e6], [1000001.0, 0, 0]], np.float32)])
    got, _ = rd.check(q, t, None, 1e-3, label="1e6 - 1")
    assert (got["idx"][:200] >= 0).all() and (got["d2"][:200] == 0).all()
    assert got["idx"][-2] == 400 and got["idx"][-1] == -2 and got["info"].tolist()[:2] == [1, 2]


def test_five_thousand_targets_in_one_cell():
    rng = np.random.default_rng(12)
    t = rng.uniform(0.05, 1.95, (5000, 3)).astype(np.float32)             # one cell of edge 2.02
    q = rng.uniform(-2.5, 4.5, (300, 3)).astype(np.float32)
    got, _ = rd.check(q, t, None, 2.0, label="one cell")
    assert int(got["info"][2]) == 1 and int(got["info"][3]) == 5000


def _hash(c, mask):
    c = np.asarray(c, np.int64) & 0xFFFFFFFF
    return int(((c[0] * 73856093) ^ (c[1] * 19349663) ^ (c[2] * 83492791)) & mask)


def test_three_far_apart_targets_in_eight_buckets():
    """m = 3: H = 8, so the 27 cells around a query fall into at most 8 buckets and most of them collide"""
    t = np.array([[0.3, 0.3, 0.3], [100.2, 0.1, 0.4], [0.2, 100.3, -0.4]], np.float32)
    rng = np.random.default_rng(13)
    q = np.concatenate([t[rng.integers(0, 3, 90)] + rng.uniform(-1.5, 1.5, (90, 3)), rng.uniform(-3, 103, (60, 3))]).astype(np.float32)
    got, _ = rd.check(q, t, None, 1.0, label="H = 8")
    assert sorted(set(got["idx"].tolist())) == [-1, 0, 1, 2]


def test_two_of_a_querys_cells_share_a_bucket():
    """hand-built: r = 1 (h = 1.01), four targets (H = 8), the query in cell (0, 0, 0).  Its neighbours (0, 1, 0) and (0, 0, 1)
    hash to ONE bucket; each holds a target 0.75 m from the query (dyadic: an exact tie), one of them twice.  Every record is
    weighed once and the tie goes to the lowest row, whichever cell it lies in."""
    assert _hash((0, 1, 0), 7) == _hash((0, 0, 1), 7) != _hash((0, 0, 0), 7)
    q = np.array([[0.5, 0.5, 0.5]], np.float32)
    in_y, in_z, far = [0.5, 1.25, 0.5], [0.5, 0.5, 1.25], [50.0, 50.0, 50.0]
    for rows in ([in_z, in_y, in_z, far], [in_y, in_z, far, in_y], [far, in_y, in_z, in_z]):
        t = np.asarray(rows, np.float32)
        assert {tuple(np.floor(r / 1.01).astype(int)) for r in t[:3].astype(np.float64) if r[0] < 10} <= {(0, 1, 0), (0, 0, 1)}
        got, _ = rd.check(q, t, None, 1.0, label="shared bucket")
        assert got["idx"].tolist() == [rows.index(far) == 0 and 1 or 0] and got["d2"].tolist() == [0.5625]
    # and a random cloud of four targets (H = 8) seen from many queries
    rng = np.random.default_rng(14)
    t4 = rng.uniform(-1.0, 2.0, (4, 3)).astype(np.float32)
    rd.check(rng.uniform(-2.0, 3.0, (500, 3)).astype(np.float32), t4, None, 1.0, label="four targets")


# ---- rows and arguments -----------------------------------------------------------------------------------------------------
def test_bad_rows_in_both_clouds():
    q, t, f, g = rd.scene(600, 700, seed=21, span=4.0, radius=1.0, G=3, bad=True)
    got, (_, idx, tab, info) = rd.check(q, t, f, 1.0, g, 3, EDGES, label="bad rows")
    assert info["bad_queries"] >= 5 and info["bad_targets"] >= 5 and int((got["idx"] == -2).sum()) == info["bad_queries"]
    assert int(tab["rows"].sum()) == 600 - info["bad_queries"]
    bad_t = np.flatnonzero(~rr.good_rows(t))
    assert not np.isin(got["idx"], bad_t).any()
    # every target bad: every good query is a miss
    got, _ = rd.check(q, np.full((40, 3), 1e8, np.float32), f, 1.0, g, 3, EDGES, label="pads only")
    assert set(got["idx"].tolist()) == {-1, -2} and int(got["info"][1]) == 40 and int(got["info"][2]) == 0


def test_optional_arguments():
    q, t, f, g = rd.scene(700, 800, seed=22, span=4.0, radius=1.0, G=64)
    rd.check(q, t, None, 1.0, g, 64, EDGES, label="no flow")
    rd.check(q, t, f, 1.0, None, 1, EDGES, label="no groups, G = 1")
    rd.check(q, t, f, 1.0, None, 5, EDGES, label="no groups, G = 5")          # every row in group 0
    got, (_, _, tab, _) = rd.check(q, t, f, 1.0, g, 64, (0.01, 0.05, 0.1, 1.0), label="G = 64, E = 4")
    assert (tab["rows"] > 0).sum() == 64
    rd.check(q, t, f, 1.0, g, 64, (), label="E = 0")
    g2 = g.copy()
    g2[::7] = np.array([-1, 64, 1 << 30, -(1 << 31)], np.int64)[np.arange(len(g2[::7])) % 4].astype(np.int32)
    got, (_, _, _, info) = rd.check(q, t, f, 1.0, g2, 64, EDGES, label="groups outside")
    assert info["bad_queries"] == len(g2[::7])
    rd.run(q, t, f, 1.0, g, 65, EDGES, expect=-1, expect_message="G must lie in [1, 64]")
    rd.run(q, t, f, 1.0, g, 3, (0.1, 0.05), expect=-1, expect_message="edges")
    rd.run(q, t, f, 2000.0, g, 3, (), expect=-1, expect_message="radius")
    rd.run(q, t, f, 1.0, g, 3, EDGES, short=1, expect=-2, expect_message="workspace")


@pytest.mark.parametrize("left_out", rd.OUTPUTS)
def test_each_output_null_in_turn(left_out):
    q, t, f, g = rd.scene(900, 1000, seed=23, span=4.0, radius=1.0, G=4)
    full = rd.run(q, t, f, 1.0, g, 4, EDGES)
    outputs = tuple(k for k in rd.OUTPUTS if k != left_out)
    got = rd.run(q, t, f, 1.0, g, 4, EDGES, outputs=outputs)
    rd.compare(got, q, t, f, 1.0, g, 4, EDGES, label=f"without {left_out}")
    for k in ("d2", "idx", "words", "info"):
        if got[k] is not None:
            assert got[k].tobytes() == full[k].tobytes(), k
    only = rd.run(q, t, f, 1.0, g, 4, EDGES, outputs=(left_out,))             # and that one alone
    key = "words" if left_out == "table" else left_out
    assert only[key].tobytes() == full[key].tobytes()
    rd.run(q, t, f, 1.0, g, 4, EDGES, outputs=(), expect=-1, expect_message="all NULL")


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_reruns_and_streams_give_identical_bits():
    """crowded buckets (the scatter's order inside a bucket is whatever the atomics made it) and a table of several workgroups"""
    q, t, f, g = rd.scene(6000, 5000, seed=31, span=3.0, radius=1.0, G=4)
    first = rd.run(q, t, f, 1.0, g, 4, EDGES)
    runs = [rd.run(q, t, f, 1.0, g, 4, EDGES, poison=p) for p in (0x00, 0xFF)]
    for s in (torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)):
        with torch.cuda.stream(s):
            runs.append(rd.run(q, t, f, 1.0, g, 4, EDGES))
    for other in runs:
        for k in ("d2", "idx", "words", "info"):
            assert other[k].tobytes() == first[k].tobytes(), k
    rd.compare(first, q, t, f, 1.0, g, 4, EDGES)
    assert int(first["info"][3]) >= 4


# ---- the integer statement ----------------------------------------------------------------------------------------------------
def test_dyadic_clouds_equal_the_integer_statement():
    hits = 0
    for kq, kf, kt, radius in rr.dyadic_clouds(400, seed=11):                  # the clouds of tests/test_residual.py
        q, f, t = rr.dyadic_floats(kq, kf, kt)
        got = rd.run(q, t, f, radius, outputs=("d2", "idx"))
        want_d2, want_idx = rr.exact_dyadic(kq, kf, kt, radius)
        assert np.array_equal(got["d2"], want_d2) and np.array_equal(got["idx"], want_idx), (len(kq), len(kt), radius)
        hits += int((want_idx >= 0).sum())
    assert hits > 2000


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _rigid_pair(seed, gt=True):
    """a synthetic.py frame pair whose destination is the rigidly moved source: dst = src + gt_flow, rounded once"""
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=seed, n_objects=6, n_min=60, n_max=400, n_background=600)
    dst = (d["points_src"].astype(np.float64) + d["gt_flow"].astype(np.float64)).astype(np.float32)
    return frame_pairs.FramePair(d["points_src"], dst, d["labels_src"], d["labels_src"].copy(), d["pose"], d["gt_flow"] if gt else None,
                                 name=f"rigid_{seed}")


@pytest.fixture(scope="module")
def rigid_directory(tmp_path_factory):
    from icp_flow_amd import frame_pairs
    root = tmp_path_factory.mktemp("rigid")
    dirs = {}
    for gt in (True, False):
        d = root / ("with_gt" if gt else "without_gt")
        d.mkdir()
        for seed in (41, 42, 43, 44, 45):
            frame_pairs.save_frame_pair(str(d / f"fp_{seed}.npz"), _rigid_pair(seed, gt))
        dirs[gt] = str(d)
    return dirs


def test_the_ground_truth_flow_leaves_only_the_rounding_of_p_plus_f():
    from icp_flow_amd import utils_eval
    fp = _rigid_pair(41)
    up = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    d2, idx, table = utils_eval.nn_residual(up(fp.points_src), up(fp.points_dst), up(fp.gt_flow), radius=2.0)
    # q = fl(p + f) and the destination row fl(p + f) computed in fp64 first: per coordinate both lie within half a float32
    # step of the exact sum, so they differ by at most one step of the largest coordinate, 2^-23 * 2^ceil(log2 max|x|)
    step = 2.0 ** -23 * 2.0 ** np.ceil(np.log2(np.abs(fp.points_dst).max()))
    d = np.sqrt(d2.cpu().numpy().astype(np.float64))
    assert (idx.cpu().numpy() >= 0).all() and d.max() <= np.sqrt(3.0) * step
    assert table.n() == len(fp.points_src) and table.hit_rate() == 1.0 and table.shares() == (1.0, 1.0) and table.bad == 0
    assert table.info["bad_targets"] == 0 and table.info["longest_bucket"] >= 1
    both = utils_eval.chamfer(up(fp.points_src) + up(fp.gt_flow), up(fp.points_dst), 2.0)
    assert both["chamfer"] <= 2 * np.sqrt(3.0) * step


def test_the_pipelines_own_flow_brings_the_matched_rows_nearer():
    from icp_flow_amd import frame_pairs
    fp = _rigid_pair(42)
    a = frame_pairs.default_args(max_points=2048)
    a.residual = 2.0
    out = frame_pairs.register_frame_pair(a, fp, DEV)
    af, ab, bf, bb = frame_pairs.frame_residual(fp, out, DEV, 2.0)
    assert af.n(3) > 100 and af.n(3) == bf.n(3) and af.n() == len(fp.points_src)
    assert af.mean(3) < bf.mean(3)
    for g in (0, 1):                                     # ground and unclustered rows do not move: the same numbers, bit for bit
        assert af.n(g) > 0 and af.words().reshape(4, -1)[g].tolist() == bf.words().reshape(4, -1)[g].tolist()
    assert ab.mean() <= bb.mean() and ab.n() == len(fp.points_dst)


def test_run_stream_with_the_flag(rigid_directory):
    from icp_flow_amd import frame_pairs
    a = frame_pairs.default_args(max_points=2048)
    plain = frame_pairs.run_stream(a, frame_pairs.list_frame_pairs(rigid_directory[True]), DEV)
    assert list(plain) == ["frame_pairs", "matched_cluster_pairs", "n_gpus", "ms_per_frame_pair", "frame_pairs_per_s", "evaluated_points",
                           "pose_sources", "epe", "accs", "accr", "outlier", "Routlier"]
    a.residual = 2.0
    blocks = {}
    for gt in (True, False):
        for in_flight in (1, 4):
            s = frame_pairs.run_stream(a, frame_pairs.list_frame_pairs(rigid_directory[gt]), DEV, in_flight=in_flight)
            assert s["frame_pairs"] == 5 and s["ms_residual_per_frame_pair"] > 0 and ("epe" in s) == gt
            assert [k for k in s if k not in ("residual", "ms_residual_per_frame_pair")] == [k for k in plain if gt or k in list(plain)[:7]]
            if gt:
                assert s["epe"] == plain["epe"] and s["matched_cluster_pairs"] == plain["matched_cluster_pairs"]
            blocks[gt, in_flight] = json.dumps(s["residual"], sort_keys=True)
    assert len(set(blocks.values())) == 1
    block = json.loads(blocks[True, 1])
    assert block["radius"] == 2.0 and block["edges"] == [0.05, 0.1] and block["groups"] == ["ground", "unclustered", "unmatched", "matched"]
    m = lambda side: block[side]["forward"]["groups"]["matched"]   # noqa: E731
    assert m("after")["n"] == m("before")["n"] > 500 and m("after")["mean"] < m("before")["mean"]
    assert block["after"]["chamfer"] < block["before"]["chamfer"]
    before, after = frame_pairs.residual_tables(block)
    assert after["forward"].mean(3) == m("after")["mean"]


def test_the_command_line_prints_the_lines(rigid_directory, capsys):
    from icp_flow_amd import frame_pairs
    frame_pairs.main([rigid_directory[False], "--max-points", "2048", "--residual"])
    text = capsys.readouterr().out
    assert "Nearest-neighbour residual, truncated at 2 m" in text and "truncated Chamfer distance" in text
    summary = json.loads(text.strip().splitlines()[-1])
    assert summary["residual"]["radius"] == 2.0 and "epe" not in summary

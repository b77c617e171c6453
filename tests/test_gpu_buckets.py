"""icpflow_seq_bucket_table on the GPU against the numpy restatement (tests/bucket_restatement.py): every count equal, every sum
within (n - 1) 2^-53 sum |x| of math.fsum -- the bound tests/test_gpu_segments.py derives for a fixed-order fp64 sum of n terms --
the table between guard words, on a poisoned workspace of exactly the size the library asks for.  Then the cross-checks
against icpflow_seq_class_table and icpflow_seq_metrics, the demo sample of G15 on the device, reruns and streams, and
run_sequences(dataset="argo") and the command line end to end with the bucket-normalised EPE on."""
import ctypes
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import argo_restatement as ar         # noqa: E402
import bucket_restatement as br       # noqa: E402
import class_restatement as cr        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
GUARD, SENTINEL, POISON = 64, -0x0123456789ABCDEF, 0xA5
CROPS = {"none": (0, 0.0, 0.0, 0.0), "xy": (1, 32.0, 32.0, 0.0), "xyz": (2, 32.0, 32.0, 0.3)}
EDGES = tuple(br.EDGES)


def enqueue(x, F, crop="xyz", G=33, edges=EDGES, class_lo=-1, poison=POISON, expect=0):
    """icpflow_seq_bucket_table on numpy inputs, on the current stream, nothing waited for: table and info between GUARD
    sentinel words, the workspace exactly workspace_bytes() long and filled with `poison`.  -> what `collect` reads"""
    from icp_flow_amd import _lib
    m, S = len(x["tim"]), len(edges) + 1
    keep = [G_(np.asarray(x["pts"], np.float64).reshape(m, 3)), G_(np.asarray(x["tim"], np.int32)), G_(np.asarray(x["cls"], np.float64)),
            G_(np.asarray(x["gt"], np.float64).reshape(m, 3)), G_(np.asarray(x["pred"], np.float32).reshape(m, 3))]
    words = G * S * 3
    out = torch.full((GUARD + words + 2 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    need = int(_lib._L.icpflow_seq_bucket_table_workspace_bytes(m, G, S))
    grid = min(max(-(-m // 2048), 1), 256)
    assert need == (-(-grid * (words + 2) * 8 // 256) * 256 if expect == 0 else 0)
    ws = torch.full((max(need, 8),), poison, dtype=torch.uint8, device=DEV)
    sp = np.asarray(edges, np.float64)
    mode, rx, ry, zmin = CROPS[crop]
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)   # noqa: E731
    rc = _lib._L.icpflow_seq_bucket_table(*[_lib.ptr(t) for t in keep], m, F, mode, rx, ry, zmin, float(class_lo), G,
                                          sp.ctypes.data_as(ctypes.c_void_p) if len(sp) else None, S, at(GUARD), at(GUARD + words),
                                          _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    assert rc == expect, (rc, _lib._L.icpflow_last_error())
    return dict(out=out, ws=ws, keep=keep, shape=(G, S), need=need)


def collect(job):
    """-> (counts [G,S], esum [G,S], ssum [G,S], kept0, outside, the table's bytes); the guard words must be untouched"""
    torch.cuda.synchronize()
    G, S = job["shape"]
    words = G * S * 3
    host = job["out"].cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + words + 2:] == SENTINEL).all(), "a guard word was written"
    body = np.ascontiguousarray(host[GUARD:GUARD + words].reshape(G, S, 3))
    esum, ssum = np.ascontiguousarray(body[:, :, 1]).view(np.float64), np.ascontiguousarray(body[:, :, 2]).view(np.float64)
    return body[:, :, 0].copy(), esum, ssum, int(host[GUARD + words]), int(host[GUARD + words + 1]), host[GUARD:GUARD + words + 2].tobytes()


def restate(x, F, crop="xyz", G=33, edges=EDGES, class_lo=-1):
    pts = np.asarray(x["pts"], np.float64)
    args = SimpleNamespace(num_frames=F, eval_ground=crop == "none", range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
    keep = (np.abs(pts[:, 0]) < 32.0) & (np.abs(pts[:, 1]) < 32.0) if crop == "xy" else None
    return br.table(args, dict(raw_points=pts, time_indice=np.asarray(x["tim"]), scene_flow=np.asarray(x["gt"], np.float64)), x["pred"], x["cls"],
                    edges, class_lo, G, keep=keep)


def check(got, want, label=""):
    """counts, kept0 and outside equal; each sum within (n - 1) 2^-53 sum |x| of math.fsum.  -> the largest error / bound seen"""
    counts, esum, ssum, kept0, outside, _ = got
    assert np.array_equal(counts, want.counts), label
    assert (kept0, outside) == (want.kept0, want.outside), label
    worst = 0.0
    for which, sums in (("e", esum), ("speed", ssum)):
        ref, bound = want.sums(which), want.bounds(which)
        with np.errstate(invalid="ignore"):
            err = np.abs(sums - ref)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(sums), nan), (label, which)
        assert (err[~nan] <= bound[~nan]).all(), (label, which, float(np.nanmax(err - bound)))
        if (bound[~nan] > 0).any():
            worst = max(worst, float((err[~nan][bound[~nan] > 0] / bound[~nan][bound[~nan] > 0]).max()))
    return worst


def make(m, F, seed, values=None, outside=False, top=2.2):
    """m rows over F frames: points on both sides of every crop threshold, class values from `values` (default: the named
    range, the specials and a few beyond), |gt| uniform over [0, top) -- every one of the 51 buckets -- and three sizes of e."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-40, 40, m), rng.uniform(-40, 40, m), rng.uniform(-0.5, 2.0, m)], axis=1)
    tim = rng.integers(0, F, size=m).astype(np.int32)
    if outside and m >= 8:
        tim[rng.choice(m, 4, replace=False)] = (-1, F, F + 7, -(1 << 31))
    if values is None:
        values = list(range(-1, 31)) + [np.nan, np.inf, -np.inf, 3.5, -2, 31, 1e9]
    cls = np.asarray(values, np.float64)[rng.integers(0, len(values), size=m)]
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gt = d * rng.uniform(0.0, top, size=(m, 1))
    d2 = rng.normal(size=(m, 3))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    pred = (gt + d2 * rng.choice([0.01, 0.07, 0.3], size=m)[:, None] * rng.uniform(0.5, 1.5, size=(m, 1))).astype(np.float32)
    return dict(pts=pts, tim=tim, cls=cls, gt=gt, pred=pred)


# ---- kernel against restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 2049])
@pytest.mark.parametrize("crop", list(CROPS))
def test_kernel_equals_the_restatement(m, crop):
    """m around a tile and into the second workgroup, all three crop modes; F = 2, and F = 5 with time indices -1, 5, 12 and
    INT_MIN among the rows; the Argoverse shape (33, 51) and the smallest one (2, 1)."""
    for k, (F, outside) in enumerate(((2, False), (5, True))):
        x = make(m, F, seed=100 * m + k, outside=outside)
        got = collect(enqueue(x, F, crop))
        want = restate(x, F, crop)
        worst = check(got, want, (m, crop, F))
        if m >= 8:
            assert got[4] == (4 if outside else 0)
        if m == 0:
            assert not got[0].any() and got[5] == bytes(8 * (33 * 51 * 3 + 2))
        if m == 2049:
            assert int(got[0].sum()) > 200 and int(got[0][32].sum()) > 0 and (got[0].sum(axis=0) > 0).sum() >= 45
            print(f"m {m} {crop} F {F}: {int(got[0].sum())} rows counted in {int((got[0] > 0).sum())} cells, largest error / bound {worst:.3f}")
        small = dict(G=2, edges=(), class_lo=5)
        check(collect(enqueue(x, F, crop, **small)), restate(x, F, crop, **small), (m, crop, F, "2x1"))


def test_grid_at_its_cap_runs_several_rounds():
    """524 288 + 777 rows: 256 workgroups of 4 waves take 1024 tiles a round, the rows need 8205: nine rounds, the last one
    with waves that have no tile."""
    m = 524288 + 777
    x = make(m, 3, seed=9)
    got = collect(enqueue(x, 3))
    worst = check(got, restate(x, 3), "cap")
    assert int(got[0].sum()) > 100000 and (got[0] > 0).sum() > 33 * 45
    print(f"m {m}: {int(got[0].sum())} rows counted, largest error / bound {worst:.4f}")


def test_the_limits_are_exact():
    """(64, 64) is 12 288 words = 96 KB of LDS and runs; (65, 2) and (2, 65) are refused with guards and poison intact."""
    x = make(3000, 2, seed=4, values=list(range(-1, 64)) + [np.nan], top=6.5)
    big = dict(G=64, edges=tuple(0.1 * k for k in range(1, 64)), class_lo=-1)
    got = collect(enqueue(x, 2, "none", **big))
    check(got, restate(x, 2, "none", **big), "64x64")
    assert (got[0].sum(axis=1) > 0).sum() >= 60 and (got[0].sum(axis=0) > 0).all() and got[0][63].sum() > 0 and got[0][:, 63].sum() > 0
    for kw in (dict(G=65, edges=(0.1,)), dict(G=2, edges=tuple(0.1 * k for k in range(1, 65)))):
        job = enqueue(x, 2, "none", expect=-3, **kw)
        torch.cuda.synchronize()
        assert job["need"] == 0 and bool((job["out"] == SENTINEL).all()) and bool((job["ws"] == POISON).all())


def test_tiles_of_64_cells_and_of_one_cell():
    """Three tiles of 64 rows: every row in a cell of its own (64 butterflies, 64 records), every row in one cell, every row in
    the last class row; then the three together, and the three together four times over so that the four waves of a workgroup
    hold records for the same cells in one round."""
    rng = np.random.default_rng(21)
    cells = [(g, s) for g in range(33) for s in range(51)]
    pick = [cells[k] for k in rng.permutation(len(cells))[:64]]

    def rows(classes, buckets):
        n = len(classes)
        gt = np.zeros((n, 3))
        gt[:, 0] = [0.04 * s + 0.04 * (0.1 + 0.8 * rng.random()) for s in buckets]
        pred = (gt + rng.normal(scale=0.05, size=(n, 3))).astype(np.float32)
        return dict(pts=np.tile([1.0, 1.0, 1.0], (n, 1)), tim=np.ones(n, np.int32), cls=np.asarray(classes, np.float64), gt=gt, pred=pred)

    tiles = [rows([g - 1 if g < 32 else np.nan for g, _ in pick], [s for _, s in pick]), rows([19] * 64, [7] * 64),
             rows([np.nan, 31, 3.5, -7] * 16, [50] * 64)]
    for k, x in enumerate(tiles):
        got = collect(enqueue(x, 2))
        check(got, restate(x, 2), f"tile {k}")
        if k == 0:
            assert int((got[0] == 1).sum()) == 64 and int(got[0].sum()) == 64
        elif k == 1:
            assert got[0][20, 7] == 64
        else:
            assert got[0][32, 50] == 64
    every = {key: np.concatenate([x[key] for x in tiles]) for key in tiles[0]}
    check(collect(enqueue(every, 2)), restate(every, 2), "three tiles")
    four = {key: np.concatenate([every[key]] * 4) for key in every}
    got = collect(enqueue(four, 2))
    check(got, restate(four, 2), "twelve tiles")
    assert got[0][20, 7] == 256 and got[0][32, 50] == 256


def test_class_values():
    """NaN, +-inf and 3.5 are `other`; so are class_lo - 1 and class_lo + G - 1; class_lo is row 0, class_lo + G - 2 row G - 2."""
    for lo, G in ((-1, 33), (4, 6)):
        values = [np.nan, np.inf, -np.inf, 3.5, lo - 1, lo, lo + G - 2, lo + G - 1, lo + 0.5, -0.0]
        n = len(values)
        x = dict(pts=np.ones((n, 3)), tim=np.ones(n, np.int32), cls=np.asarray(values), gt=np.tile([0.01, 0.0, 0.0], (n, 1)),
                 pred=np.zeros((n, 3), np.float32))
        got = collect(enqueue(x, 2, G=G, class_lo=lo))
        rows = got[0].sum(axis=1)
        in_range = 1 if lo <= 0 <= lo + G - 2 else 0                      # (-0.0 is the integer 0)
        assert rows[0] == 1 and rows[G - 2] == 1 and rows[G - 1] == n - 2 - in_range and int(rows.sum()) == n
        check(got, restate(x, 2, G=G, class_lo=lo), (lo, G))


@pytest.mark.parametrize("F", [2, 5])
def test_time_indices_outside_are_counted_and_nothing_else(F):
    """Time indices -1, F, F + 7, INT_MIN and INT_MAX are `outside`; 0 is frame 0 (kept0); 1 .. F - 1 count."""
    tim = np.array([-1, F, F + 7, -(1 << 31), (1 << 31) - 1, 0, 0] + list(range(1, F)) * 3, np.int32)
    n = len(tim)
    rng = np.random.default_rng(F)
    x = dict(pts=np.ones((n, 3)), tim=tim, cls=rng.integers(-1, 31, n).astype(np.float64), gt=rng.uniform(0, 1, (n, 3)), pred=np.zeros((n, 3), np.float32))
    got = collect(enqueue(x, F))
    assert (got[3], got[4]) == (2, 5) and int(got[0].sum()) == 3 * (F - 1)
    check(got, restate(x, F), F)


def test_rows_on_an_edge_land_in_the_upper_bucket():
    """gt = (edge, 0, 0) and one ulp to either side, zero prediction: sqrt(edge * edge) is edge in binary floating point -- the
    same fp64 operations on the host and on the device -- so |gt| = edge, and `>=` puts the row into the bucket that STARTS
    at the edge.  A NaN speed is bucket 0."""
    at = (0, 1, 24, 49)
    xs = [f(br.EDGES[k]) for k in at for f in (lambda v: np.nextafter(v, 0.0), lambda v: v, lambda v: np.nextafter(v, 10.0))]
    assert all(np.sqrt(np.float64(v) * np.float64(v)) == v for v in xs)
    n = len(xs) + 1
    gt = np.zeros((n, 3))
    gt[:-1, 0] = xs
    gt[-1] = (np.nan, 0.0, 0.0)
    x = dict(pts=np.ones((n, 3)), tim=np.ones(n, np.int32), cls=np.arange(n, dtype=np.float64), gt=gt, pred=np.zeros((n, 3), np.float32))
    got = collect(enqueue(x, 2))
    for i, v in enumerate(xs):
        k = at[i // 3]
        s = k + (0 if i % 3 == 0 else 1)                                  # below the edge: bucket k; on it and above: bucket k + 1
        assert got[0][i + 1].sum() == 1 and got[0][i + 1, s] == 1 and got[1][i + 1, s] == v and got[2][i + 1, s] == v, (i, v)
    assert got[0][n, 0] == 1 and np.isnan(got[2][n, 0])
    check(got, restate(x, 2), "edges")


# ---- cross-checks with the two kernels beside it -------------------------------------------------------------------------------
def test_counts_equal_the_class_table_and_the_metrics():
    """With ARGO_SPEED_EDGES (S = 3) the counts equal icpflow_seq_class_table's summed over its error splits, exactly; with the
    51 buckets the total over all cells equals icpflow_seq_metrics' `overall` count; kept0 is the same number in all three."""
    from icp_flow_amd import utils_eval
    x = make(30011, 4, seed=33, top=0.5)
    data = dict(raw_points=G_(x["pts"]), time_indice=G_(x["tim"]), scene_flow=G_(x["gt"]), classes=G_(x["cls"]),
                sd_labels=G_(np.zeros(len(x["tim"]), np.int32)), fb_labels=G_(np.zeros(len(x["tim"]), np.int32)))
    pred = G_(x["pred"])
    for setting in ("default", "ground"):
        args = SimpleNamespace(**dict(ar.SETTINGS[setting], num_frames=4))
        classes = utils_eval.class_table(args, data, pred)
        three = utils_eval.bucket_table(args, data, pred, speed_edges=utils_eval.ARGO_SPEED_EDGES)
        assert three.counts.shape == (33, 3) and np.array_equal(three.counts, classes.counts.sum(axis=2)) and (three.counts.sum(axis=0) > 0).all()
        full = utils_eval.bucket_table(args, data, pred)
        table, _, kept0, outside = utils_eval.sequence_table(args, data, pred)
        assert full.counts.shape == (33, 51) and int(full.counts.sum()) == int(table[0, 0, 0]) == int(three.counts.sum()) > 1000
        assert full.kept0 == three.kept0 == classes.kept0 == kept0 and outside == 0
    data["time_indice"] = G_(np.where(np.arange(len(x["tim"])) == 5, 9, x["tim"]).astype(np.int32))
    with pytest.raises(ValueError, match=r"1 points have a time index outside \[0, 4\)"):
        utils_eval.bucket_table(args, data, pred)


# ---- the demo sample on the device ----------------------------------------------------------------------------------------
def _metric_close(got, ref, n, label):
    for name in list(br.GROUP_NAMES) + ["OTHER"]:
        for key in ("n_static", "n_dynamic", "buckets_used"):
            assert got[name][key] == ref[name][key], (label, name, key)
        for key in ("static", "dynamic"):
            a, b = got[name][key], ref[name][key]
            assert math.isnan(a) == math.isnan(b) and (math.isnan(a) or abs(a - b) <= br.metric_tolerance(n) * abs(b)), (label, name, key, a, b)
    for key in ("mean_static", "mean_dynamic"):
        a, b = got[key], ref[key]
        assert math.isnan(a) == math.isnan(b) and (math.isnan(a) or abs(a - b) <= br.metric_tolerance(n) * abs(b)), (label, key, a, b)


def test_demo_sample_equals_the_restatement():
    """utils_loading.argo_sample and utils_eval.bucket_table on the demo sample of G15 (126 598 rows) under its three settings:
    the whole table is the restatement's, the total the REFERENCE's recorded `overall` count, and bucketed_epe the
    restatement's metric within the summation bound (tests/bucket_restatement.py: metric_tolerance)."""
    from icp_flow_amd import utils_eval, utils_loading
    arrays, pred = ar.file_arrays(ar.DEMO)
    data = utils_loading.argo_sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"], arrays["pc1_flows_valid_idx"],
                                     arrays["pc2_flows_valid_idx"])
    s, _ = cr.fixture_sample(ar.DEMO)
    g = ar.load(ar.DEMO)
    names = [str(n) for n in g["meter_names"]]
    for setting in ar.SETTINGS:
        args = ar.setting_args(setting)
        t = utils_eval.bucket_table(args, data, G_(pred))
        want = br.table(args, s, pred, s["classes"])
        worst = check((t.counts, t.esum, t.ssum, t.kept0, 0, b""), want, setting)
        n = int(t.counts.sum())
        assert n == int(g[setting + "_num"][names.index("overall_1")]) and n > 10000
        got = utils_eval.bucketed_epe(t)
        _metric_close(got, br.metric(want), n, setting)
        print(f"{setting}: {n} rows in {int((t.counts > 0).sum())} cells, largest error / bound {worst:.3f}, mean static {got['mean_static']:.6f}, "
              f"mean dynamic {got['mean_dynamic']:.6f}")


def test_reruns_and_two_streams_are_bit_identical():
    """The same call twice on workspaces poisoned differently, and two samples enqueued on two streams before either is waited
    for, against the same two one after the other on one stream."""
    cases = [(make(70000, 2, seed=61), 2), (make(30011, 4, seed=62, outside=True), 4)]
    first = [collect(enqueue(x, F))[5] for x, F in cases]
    again = [collect(enqueue(x, F, poison=0x3C))[5] for x, F in cases]
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    jobs = []
    torch.cuda.synchronize()
    for (x, F), s in zip(cases, streams):
        with torch.cuda.stream(s):
            jobs.append(enqueue(x, F, poison=0xFF))
    both = [collect(j)[5] for j in jobs]
    assert first == again == both


def test_an_empty_sample_succeeds_with_a_zero_table():
    from icp_flow_amd import utils_eval
    e3 = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    data = dict(raw_points=e3, time_indice=torch.zeros(0, dtype=torch.int32, device=DEV), scene_flow=e3,
                classes=torch.zeros(0, dtype=torch.float64, device=DEV))
    t = utils_eval.bucket_table(ar.setting_args("argo"), data, e3.to(torch.float32))
    assert t.counts.shape == (33, 51) and not t.counts.any() and not t.esum.any() and not t.ssum.any() and t.kept0 == 0
    assert math.isnan(utils_eval.bucketed_epe(t)["mean_dynamic"])


# ---- run_sequences --------------------------------------------------------------------------------------------------------
BACKGROUND = (5, 8, 9, 13, 21, 22)


@pytest.fixture(scope="module")
def argo_dir(tmp_path_factory):
    """tests/test_gpu_classes.py's two-file directory, built the same way, under a split directory of the Argoverse tree"""
    from icp_flow_amd import synthetic
    tmp = os.path.join(str(tmp_path_factory.mktemp("argo_buckets")), "val_zero_flow", "log0")
    os.makedirs(tmp)
    arrays, _ = ar.file_arrays(ar.DEMO)
    np.savez(os.path.join(tmp, "a_demo.npz"), **arrays)
    d = synthetic.make_frame_pair(seed=12, n_objects=6, n_min=600, n_max=1500, n_background=600)
    rng = np.random.default_rng(16)
    n, m1, m2 = 7000, len(d["points_src"]), len(d["points_dst"])
    v1, keep2 = rng.permutation(n)[:m1], np.zeros(n, bool)       # an unsorted index list and a boolean mask
    keep2[rng.choice(n, m2, replace=False)] = True
    pc1, pc2, flow = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
    classes = np.full(n, 99, np.int8)
    pc1[v1], pc2[keep2], flow[v1] = d["points_src"], d["points_dst"], d["gt_flow"]
    classes[v1] = np.array(list(BACKGROUND) + [-1, 0, 19, 19, 17, 3])[rng.integers(0, 12, size=m1)]
    np.savez(os.path.join(tmp, "b_synthetic.npz"), pc1=pc1, pc2=pc2, gt_flow_0_1=flow, pc1_classes=classes, pc1_flows_valid_idx=v1,
             pc2_flows_valid_idx=keep2)
    return tmp


def _same_meters(got, ref):
    from icp_flow_amd import utils_eval
    assert list(got) == list(ref)
    for name in got:
        assert got[name].num == ref[name].num and got[name].num_data == ref[name].num_data, name
        for m in utils_eval.METRIC_NAMES:
            for field in ("_sum", "_avg", "_data"):
                a, b = np.asarray(getattr(got[name], m + field), np.float64), np.asarray(getattr(ref[name], m + field), np.float64)
                assert a.tobytes() == b.tobytes(), (name, m, field)


def test_run_sequences_end_to_end(argo_dir, capsys):
    """run_sequences(dataset="argo") with the bucket table and the saving on: the meters are bit for bit those of a run without
    the flag; the accumulated counts are the sum of the per-file restatements on the SAVED flows, and bucketed_epe is the
    restatement's metric on them within the summation bound; with the class table on as well both come back; the command line
    prints the block after the reference's table and carries `bucketed_epe` in its JSON line."""
    from icp_flow_amd import frame_pairs, utils_eval
    paths = frame_pairs.list_frame_pairs(argo_dir)
    assert len(paths) == 2 and all(frame_pairs.is_argo(p) for p in paths)
    a = frame_pairs.default_args(cluster="dbscan", speed=1.67)
    for k, v in dict(ar.SETTINGS["argo"], num_frames=2).items():
        setattr(a, k, v)
    plain = frame_pairs.run_sequences(a, paths, DEV, dataset="argo")
    assert "bucket_table" not in plain and "bucketed_epe" not in plain
    a.bucket_table, a.class_table, a.save_flows = True, "meta", True
    res = frame_pairs.run_sequences(a, paths, DEV, dataset="argo", rank=0, world=1)
    assert res["sequences"] == 2 and "class_table" in res and "threeway" in res
    _same_meters(res["metrics"], plain["metrics"])
    table = res["bucket_table"]
    want = br.Cells(33, 51)
    for path in paths:
        with np.load(path) as z:
            s = ar.sample(z["pc1"], z["pc2"], z["gt_flow_0_1"], z["pc1_classes"], z["pc1_flows_valid_idx"], z["pc2_flows_valid_idx"], BACKGROUND)
            v1 = ar.index_list(z["pc1_flows_valid_idx"])
            cls1 = z["pc1_classes"][v1].astype(np.float64)
        s["raw_points"] = s["raw_points"].astype(np.float32)
        m2 = len(s["time_indice"]) - len(v1)
        with np.load(frame_pairs.flow_file(path)) as z:
            saved = z["scene_flow"]
        flow_seq = saved.astype(np.float32)
        assert np.array_equal(flow_seq.astype(np.float64), saved) and not flow_seq[:m2].any()
        want.extend(br.table(a, s, flow_seq, np.concatenate([np.full(m2, np.nan), cls1])))
    assert np.array_equal(table.counts, want.counts) and table.kept0 == want.kept0
    assert np.array_equal(table.counts.sum(axis=1), res["class_table"].counts.sum(axis=(1, 2)))
    n = int(table.counts.sum())
    assert n > 60000 and int(table.counts[32].sum()) == 0 and int(table.counts[20].sum()) > 0       # REGULAR_VEHICLE (file value 19)
    # each accumulated sum: the additions of a cell's n values in some fixed tree (kernel, then file after file)
    check((table.counts, table.esum, table.ssum, table.kept0, 0, b""), want, "accumulated")
    got = res["bucketed_epe"]
    assert json.dumps(got) == json.dumps(utils_eval.bucketed_epe(table))
    _metric_close(got, br.metric(want), n, "run_sequences")
    assert got["CAR"]["n_static"] + got["CAR"]["n_dynamic"] == int(table.counts[20].sum())
    capsys.readouterr()
    # the command line: the reference's table, then the block; the JSON line carries the metric and not the table
    frame_pairs.main([argo_dir, "--protocol", "reference", "--dataset", "argo", "--cluster", "dbscan", "--speed", "1.67", "--range-x", "10000",
                      "--range-y", "10000", "--range-z", "-10000", "--ground-slack", "0", "--bucketed-epe"])
    printed = capsys.readouterr().out.split("\n")
    lines = utils_eval.format_metric_table(res["metrics"], 2).split("\n") + utils_eval.format_bucketed_epe(got).split("\n")
    start = printed.index(lines[0])
    assert printed[start:start + len(lines)] == lines
    summary = json.loads(printed[start + len(lines)])
    assert "bucket_table" not in summary and "class_table" not in summary and "threeway" not in summary
    assert json.dumps(summary["bucketed_epe"]) == json.dumps(got)
    a.class_table = None
    with pytest.raises(ValueError, match="bucket_table goes with dataset='argo'"):
        frame_pairs.run_sequences(a, [], DEV, dataset="pca")

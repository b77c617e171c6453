"""icpflow_seq_class_table on the GPU against the numpy restatement (tests/class_restatement.py): every count equal, every sum
within (n - 1) 2^-53 sum |x| of math.fsum -- the bound tests/test_gpu_segments.py derives for a sequential sum of n terms -- the
table between guard words, on a poisoned workspace of exactly the size the library asks for.  Then the g15 fixtures on the
device against the REFERENCE's recorded counts and means, reruns and streams, and run_sequences(dataset="argo") end to end
with the class table on."""
import contextlib
import ctypes
import io
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
import class_restatement as cr        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
GUARD, SENTINEL, POISON = 64, -0x0123456789ABCDEF, 0xA5
CROPS = {"none": (0, 0.0, 0.0, 0.0), "xy": (1, 32.0, 32.0, 0.0), "xyz": (2, 32.0, 32.0, 0.3)}
ARGO = dict(G=33, S=3, E=3, speed=cr.SPEED_EDGES, error=cr.ERROR_EDGES, class_lo=-1)


def enqueue(x, F, crop="xyz", G=33, S=3, E=3, speed=cr.SPEED_EDGES, error=cr.ERROR_EDGES, class_lo=-1, poison=POISON, expect=0):
    """icpflow_seq_class_table on numpy inputs, on the current stream, nothing waited for: table and info between GUARD
    sentinel words, the workspace exactly workspace_bytes() long and filled with `poison`.  -> what `collect` reads"""
    from icp_flow_amd import _lib
    m = len(x["tim"])
    keep = [G_(np.asarray(x["pts"], np.float64).reshape(m, 3)), G_(np.asarray(x["tim"], np.int32)), G_(np.asarray(x["cls"], np.float64)),
            G_(np.asarray(x["gt"], np.float64).reshape(m, 3)), G_(np.asarray(x["pred"], np.float32).reshape(m, 3))]
    words = G * S * (E + 2)
    out = torch.full((GUARD + words + 2 + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    need = int(_lib._L.icpflow_seq_class_table_workspace_bytes(m, G, S, E))
    ws = torch.full((max(need, 8),), poison, dtype=torch.uint8, device=DEV)
    sp, er = np.asarray(speed, np.float64), np.asarray(error, np.float64)
    assert len(sp) == S - 1 and len(er) == E - 1
    mode, rx, ry, zmin = CROPS[crop]
    at = lambda k: ctypes.c_void_p(out.data_ptr() + 8 * k)   # noqa: E731
    rc = _lib._L.icpflow_seq_class_table(*[_lib.ptr(t) for t in keep], m, F, mode, rx, ry, zmin, float(class_lo), G,
                                         sp.ctypes.data_as(ctypes.c_void_p) if len(sp) else None, S,
                                         er.ctypes.data_as(ctypes.c_void_p) if len(er) else None, E, at(GUARD), at(GUARD + words),
                                         _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    assert rc == expect, (rc, _lib._L.icpflow_last_error())
    return dict(out=out, ws=ws, keep=keep, shape=(G, S, E), need=need)


def collect(job):
    """-> (counts [G,S,E], esum [G,S], ssum [G,S], kept0, outside, the table's bytes); the guard words must be untouched"""
    torch.cuda.synchronize()
    G, S, E = job["shape"]
    words = G * S * (E + 2)
    host = job["out"].cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + words + 2:] == SENTINEL).all(), "a guard word was written"
    body = np.ascontiguousarray(host[GUARD:GUARD + words].reshape(G, S, E + 2))
    esum, ssum = np.ascontiguousarray(body[:, :, E]).view(np.float64), np.ascontiguousarray(body[:, :, E + 1]).view(np.float64)
    return body[:, :, :E].copy(), esum, ssum, int(host[GUARD + words]), int(host[GUARD + words + 1]), host[GUARD:GUARD + words + 2].tobytes()


def restate(x, F, crop="xyz", G=33, S=3, E=3, speed=cr.SPEED_EDGES, error=cr.ERROR_EDGES, class_lo=-1):
    pts = np.asarray(x["pts"], np.float64)
    args = SimpleNamespace(num_frames=F, eval_ground=crop == "none", range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
    keep = (np.abs(pts[:, 0]) < 32.0) & (np.abs(pts[:, 1]) < 32.0) if crop == "xy" else None
    return cr.table(args, dict(raw_points=pts, time_indice=np.asarray(x["tim"]), scene_flow=np.asarray(x["gt"], np.float64)), x["pred"], x["cls"],
                    tuple(speed), tuple(error), class_lo, G, keep=keep)


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


def make(m, F, seed, values=None, outside=False, edges=(0.05, 0.1, 0.2)):
    """m rows over F frames: points on both sides of every crop threshold, class values from `values` (default: the named
    range, the specials and a few beyond), |gt| and e spread over every bucket and split."""
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
    top = [0.0] + list(edges) + [2.0]
    k = rng.integers(0, len(top) - 1, size=m)
    gt = d * rng.uniform(np.asarray(top)[k], np.asarray(top)[k + 1])[:, None]
    d2 = rng.normal(size=(m, 3))
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    pred = (gt + d2 * rng.choice([0.01, 0.07, 0.3], size=m)[:, None] * rng.uniform(0.5, 1.5, size=(m, 1))).astype(np.float32)
    return dict(pts=pts, tim=tim, cls=cls, gt=gt, pred=pred)


# ---- kernel against restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 2049])
@pytest.mark.parametrize("crop", list(CROPS))
def test_kernel_equals_the_restatement(m, crop):
    """m around a tile and into the second workgroup, all three crop modes; F = 2, and F = 5 with time indices -1 and 5 among
    the rows; the Argoverse shape (33, 3, 3) and the smallest one (2, 1, 1)."""
    for k, (F, outside) in enumerate(((2, False), (5, True))):
        x = make(m, F, seed=100 * m + k, outside=outside)
        got = collect(enqueue(x, F, crop))
        want = restate(x, F, crop)
        worst = check(got, want, (m, crop, F))
        if m >= 8:
            assert got[4] == (4 if outside else 0)
        if m == 2049:
            assert int(got[0].sum()) > 200 and int(got[0][32].sum()) > 0 and (got[0].sum(axis=(0, 2)) > 0).all()
            print(f"m {m} {crop} F {F}: {int(got[0].sum())} rows counted, largest error / bound {worst:.3f}")
        small = dict(G=2, S=1, E=1, speed=(), error=(), class_lo=5)
        check(collect(enqueue(x, F, crop, **small)), restate(x, F, crop, **small), (m, crop, F, "2x1x1"))


def test_grid_at_its_cap_runs_the_wave_loop_twice():
    """524 288 + 777 rows: 256 workgroups of 4 waves take 1024 tiles a round, the rows need 8205."""
    m = 524288 + 777
    x = make(m, 3, seed=9)
    got = collect(enqueue(x, 3))
    worst = check(got, restate(x, 3), "cap")
    assert int(got[0].sum()) > 100000
    print(f"m {m}: {int(got[0].sum())} rows counted, largest error / bound {worst:.4f}")


def test_the_word_limit_is_exact():
    """(64, 2, 6) is exactly 1024 words and runs; (64, 2, 7) is refused with guards and poison intact."""
    x = make(700, 2, seed=4, values=list(range(-1, 64)) + [np.nan])
    big = dict(G=64, S=2, E=6, speed=(0.1,), error=(0.02, 0.05, 0.1, 0.2, 0.4), class_lo=-1)
    got = collect(enqueue(x, 2, "none", **big))
    check(got, restate(x, 2, "none", **big), "64x2x6")
    assert (got[0].sum(axis=(1, 2)) > 0).sum() >= 60
    job = enqueue(x, 2, "none", G=64, S=2, E=7, speed=(0.1,), error=(0.02, 0.05, 0.1, 0.2, 0.4, 0.8), class_lo=-1, expect=-3)
    torch.cuda.synchronize()
    assert job["need"] == 0 and bool((job["out"] == SENTINEL).all()) and bool((job["ws"] == POISON).all())


def test_tiles_of_64_cells_of_one_cell_and_of_the_other_row():
    """Three tiles of 64 rows: every row in a cell of its own (64 butterflies), every row in one cell, every row in the
    last class row; then the three together, so that a wave meets them one after the other."""
    rng = np.random.default_rng(21)
    cells = [(g, s) for g in range(33) for s in range(3)]
    pick = [cells[k] for k in rng.permutation(len(cells))[:64]]
    mags = {0: 0.02, 1: 0.1, 2: 0.7}

    def rows(classes, buckets):
        n = len(classes)
        gt = np.zeros((n, 3))
        gt[:, 0] = [mags[s] * (1 + 0.1 * rng.random()) for s in buckets]
        pred = (gt + rng.normal(scale=0.05, size=(n, 3))).astype(np.float32)
        return dict(pts=np.tile([1.0, 1.0, 1.0], (n, 1)), tim=np.ones(n, np.int32), cls=np.asarray(classes, np.float64), gt=gt, pred=pred)

    tiles = [rows([g - 1 if g < 32 else np.nan for g, _ in pick], [s for _, s in pick]), rows([18] * 64, [1] * 64),
             rows([np.nan, 31, 3.5, -7] * 16, [2] * 64)]
    for k, x in enumerate(tiles):
        got = collect(enqueue(x, 2))
        check(got, restate(x, 2), f"tile {k}")
        n = got[0].sum(axis=2)
        if k == 0:
            assert int((n == 1).sum()) == 64 and int(n.sum()) == 64
        elif k == 1:
            assert n[19, 1] == 64
        else:
            assert n[32, 2] == 64
    every = {key: np.concatenate([x[key] for x in tiles]) for key in tiles[0]}
    check(collect(enqueue(every, 2)), restate(every, 2), "three tiles")


def test_class_values():
    """NaN, +-inf and 3.5 are `other`; so are class_lo - 1 and class_lo + G - 1; class_lo is row 0, class_lo + G - 2 row G - 2."""
    for lo, G in ((-1, 33), (4, 6)):
        values = [np.nan, np.inf, -np.inf, 3.5, lo - 1, lo, lo + G - 2, lo + G - 1, lo + 0.5, -0.0]
        n = len(values)
        x = dict(pts=np.ones((n, 3)), tim=np.ones(n, np.int32), cls=np.asarray(values), gt=np.tile([0.01, 0.0, 0.0], (n, 1)),
                 pred=np.zeros((n, 3), np.float32))
        got = collect(enqueue(x, 2, G=G, class_lo=lo))
        rows = got[0].sum(axis=(1, 2))
        in_range = 1 if lo <= 0 <= lo + G - 2 else 0                      # (-0.0 is the integer 0)
        assert rows[0] == 1 and rows[G - 2] == 1 and rows[G - 1] == n - 2 - in_range and int(rows.sum()) == n
        check(got, restate(x, 2, G=G, class_lo=lo), (lo, G))


def test_rows_on_an_edge_land_in_the_upper_bucket():
    """gt = (edge, 0, 0) and one ulp to either side, zero prediction: sqrt(edge * edge) is edge in binary floating point, so
    |gt| = e = edge, and `>=` puts the row into the bucket and the split that START at the edge."""
    edges = sorted(set(cr.SPEED_EDGES) | set(cr.ERROR_EDGES))
    xs = [f(edge) for edge in edges for f in (lambda v: np.nextafter(v, 0.0), lambda v: v, lambda v: np.nextafter(v, 1.0))]
    assert all(np.sqrt(np.float64(v) * np.float64(v)) == v for v in xs)
    n = len(xs)
    gt = np.zeros((n, 3))
    gt[:, 0] = xs
    x = dict(pts=np.ones((n, 3)), tim=np.ones(n, np.int32), cls=np.arange(n, dtype=np.float64), gt=gt, pred=np.zeros((n, 3), np.float32))
    got = collect(enqueue(x, 2))
    for i, v in enumerate(xs):
        s, k = sum(v >= edge for edge in cr.SPEED_EDGES), sum(v >= edge for edge in cr.ERROR_EDGES)
        assert got[0][i + 1, s, k] == 1 and got[1][i + 1, s] == v and got[2][i + 1, s] == v, (i, v)
    at = {edge: xs.index(edge) + 1 for edge in edges}
    assert got[0][at[0.05], 1, 1] == 1 and got[0][at[0.05] - 1, 0, 0] == 1           # 0.05: both lists
    assert got[0][at[0.1], 1, 2] == 1 and got[0][at[0.1] - 1, 1, 1] == 1             # 0.1: an error edge
    assert got[0][at[0.2], 2, 2] == 1 and got[0][at[0.2] - 1, 1, 2] == 1             # 0.2: a speed edge
    check(got, restate(x, 2), "edges")


# ---- the g15 fixtures on the device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ar.SYNTHETIC + (ar.DEMO,))
def test_g15_marginals_equal_the_reference(name):
    """utils_loading.argo_sample's `classes` and utils_eval.class_table under the three recorded settings: the marginals'
    row counts are the reference's <setting>_num, sum / count within 1e-12 (relative) of its <setting>_avg[:, 0], as on the
    CPU; and the whole table is the restatement's."""
    from icp_flow_amd import utils_eval, utils_loading
    arrays, pred = ar.file_arrays(name)
    data = utils_loading.argo_sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"], arrays["pc1_flows_valid_idx"],
                                     arrays["pc2_flows_valid_idx"])
    s, _ = cr.fixture_sample(name)
    assert data["classes"].dtype == torch.float64 and data["classes"].is_cuda
    assert np.array_equal(data["classes"].cpu().numpy(), s["classes"], equal_nan=True)
    for k in ar.SAMPLE_KEYS:
        assert np.array_equal(data[k].cpu().numpy(), s[k].astype(data[k].cpu().numpy().dtype)), k
    for setting in ar.SETTINGS:
        args = ar.setting_args(setting)
        t = utils_eval.class_table(args, data, G_(pred))
        worst = cr.check_against_recorded(name, setting, t.counts, t.esum)
        want = cr.table(args, s, pred, s["classes"])
        check((t.counts, t.esum, t.ssum, t.kept0, 0, b""), want, (name, setting))
        print(f"{name} {setting}: {int(t.counts.sum())} rows, largest relative difference of a mean {worst:.3e}")


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


# ---- run_sequences --------------------------------------------------------------------------------------------------------
BACKGROUND = (5, 8, 9, 13, 21, 22)


@pytest.fixture(scope="module")
def argo_dir(tmp_path_factory):
    """tests/test_gpu_argo.py's two-file directory, built the same way, under a split directory of the Argoverse tree"""
    from icp_flow_amd import synthetic
    tmp = os.path.join(str(tmp_path_factory.mktemp("argo_classes")), "val_zero_flow", "log0")
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
    classes[v1] = np.array(list(BACKGROUND) + [-1, 0, 18, 18, 18, 16])[rng.integers(0, 12, size=m1)]
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


def test_run_sequences_end_to_end(argo_dir, monkeypatch, capsys, tmp_path):
    """run_sequences(dataset="argo") with the class table and the saving on: the accumulated counts are the sum of the
    per-file restatements on the flows the registration returned; FD / FS / BS lie within the summation bound of the
    reference's dynamic_fg_0 / static_fg_0 / static_bg_0 means -- both are sums of the same n non-negative values in different
    orders, each within (n - 1) 2^-53 of the exact sum, plus the division, the meter's multiplication by its weight, its
    addition and its division: 2 (n + 4) 2^-53 relative; the meters are bit for bit those of a run without the flag; the
    saved files hold the float64 widening of the flows and the poses; the command line prints the lines."""
    from icp_flow_amd import frame_pairs, utils_eval
    paths = frame_pairs.list_frame_pairs(argo_dir)
    assert len(paths) == 2 and all(frame_pairs.is_argo(p) for p in paths)
    a = frame_pairs.default_args(cluster="dbscan", speed=1.67)
    for k, v in dict(ar.SETTINGS["argo"], num_frames=2).items():
        setattr(a, k, v)
    plain = frame_pairs.run_sequences(a, paths, DEV, dataset="argo")
    assert "class_table" not in plain and "threeway" not in plain and "ms_save_per_sequence" not in plain
    flows, real = [], frame_pairs.register_frame_pair

    def spy(args, fp, device, gap=None):
        out = real(args, fp, device, gap)
        flows.append(out["flow"])
        return out

    monkeypatch.setattr(frame_pairs, "register_frame_pair", spy)
    a.class_table, a.save_flows = "meta", True
    res = frame_pairs.run_sequences(a, paths, DEV, dataset="argo", rank=0, world=1)
    monkeypatch.undo()
    assert res["sequences"] == 2 and len(flows) == 2 and res["ms_save_per_sequence"] > 0
    _same_meters(res["metrics"], plain["metrics"])
    table = res["class_table"]
    want_counts, want_kept0 = np.zeros((33, 3, 3), np.int64), 0
    for path, flow in zip(paths, flows):
        with np.load(path) as z:
            s = ar.sample(z["pc1"], z["pc2"], z["gt_flow_0_1"], z["pc1_classes"], z["pc1_flows_valid_idx"], z["pc2_flows_valid_idx"], BACKGROUND)
            v1 = ar.index_list(z["pc1_flows_valid_idx"])
            cls1 = z["pc1_classes"][v1].astype(np.float64)
        s["raw_points"] = s["raw_points"].astype(np.float32)
        m2 = len(s["time_indice"]) - len(v1)
        flow_seq = np.concatenate([np.zeros((m2, 3), np.float32), flow.cpu().numpy()])
        c = cr.table(a, s, flow_seq, np.concatenate([np.full(m2, np.nan), cls1]))
        want_counts, want_kept0 = want_counts + c.counts, want_kept0 + c.kept0
        # the saved file: the flow widened, zeros for frame 0, and two identity poses, next to the split
        side = frame_pairs.flow_file(path)
        assert side == path.replace("val_zero_flow", "val_icp_flow_ego_zero_flow")
        with np.load(side) as z:
            assert sorted(z.files) == ["ego_motion", "scene_flow"]
            assert z["scene_flow"].dtype == np.float64 and np.array_equal(z["scene_flow"], flow_seq.astype(np.float64))
            assert z["ego_motion"].dtype == np.float64 and np.array_equal(z["ego_motion"], np.stack([np.eye(4)] * 2))
    assert np.array_equal(table.counts, want_counts) and table.kept0 == want_kept0
    assert int(table.counts[32].sum()) == 0 and int(table.counts[19].sum()) > 0            # REGULAR_VEHICLE (file value 18)
    tw = res["threeway"]
    assert tw == table.threeway()
    for part, name in (("FD", "dynamic_fg_0"), ("FS", "static_fg_0"), ("BS", "static_bg_0")):
        meter = res["metrics"][name]
        n = tw["n_" + part]
        print(f"{part}: {tw[part]!r} (n {n}) against {name}.epe_avg {meter.epe_avg!r}")
        assert n == int(meter.num) and n > 0
        assert abs(tw[part] - meter.epe_avg) <= 2 * (n + 4) * cr.U * meter.epe_avg
    assert tw["mean"] == (tw["FD"] + tw["FS"] + tw["BS"]) / 3.0
    # the command line: the reference's table, then the class lines and the three-way line; the JSON line carries both
    metrics_file = str(tmp_path / "metrics.npz")
    frame_pairs.main([argo_dir, "--protocol", "reference", "--dataset", "argo", "--cluster", "dbscan", "--speed", "1.67", "--range-x", "10000",
                      "--range-y", "10000", "--range-z", "-10000", "--ground-slack", "0", "--class-table", "fine", "--save-metrics", metrics_file])
    printed = capsys.readouterr().out.split("\n")
    lines = utils_eval.format_metric_table(res["metrics"], 2).split("\n") + utils_eval.format_class_table(table, fine=True).split("\n")
    start = printed.index(lines[0])
    assert printed[start:start + len(lines)] == lines
    summary = json.loads(printed[start + len(lines)])
    assert summary["class_table"]["rows"] == list(utils_eval.ARGO_ROW_NAMES) and summary["class_table"]["counts"] == table.counts.tolist()
    assert summary["threeway"] == tw
    with np.load(metrics_file) as z:
        assert len(z.files) == 90 and z["EPE3Doverall_0"].shape == (1, 2)
        assert np.array_equal(z["EPE3Ddynamic_fg_0"][0], np.asarray(res["metrics"]["dynamic_fg_0"].epe_data, np.float64))


def test_an_empty_sample_succeeds_with_a_zero_table():
    from icp_flow_amd import utils_eval
    e3 = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    data = dict(raw_points=e3, time_indice=torch.zeros(0, dtype=torch.int32, device=DEV), scene_flow=e3,
                classes=torch.zeros(0, dtype=torch.float64, device=DEV))
    t = utils_eval.class_table(ar.setting_args("argo"), data, e3.to(torch.float32))
    assert t.counts.shape == (33, 3, 3) and not t.counts.any() and not t.esum.any() and not t.ssum.any() and t.kept0 == 0
    assert math.isnan(t.threeway()["mean"])

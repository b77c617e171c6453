"""The sequence evaluation on the GPU (icpflow_seq_gt_flow, icpflow_seq_metrics and their Python mirrors) against the g13
fixtures -- the reference's own utils_loading / utils_eval.calculate_metrics run on the CPU, tools/gen_golden_seqeval.py --
and against a plain numpy restatement (tests/seqeval_restatement.py) on the shapes where a reduction can go wrong."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqeval_restatement as sr      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURES = ["g13_seqeval_f3_f32", "g13_seqeval_f3_f64", "g13_seqeval_f5_f32", "g13_seqeval_f5_f64"]
G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731


@pytest.mark.parametrize("name", FIXTURES)
def test_scene_flow_against_g13(name):
    """Every component of the ground-truth flow within 64 * 2^-53 * M of the reference's, M = max |p| + max |t_ego| + max |t_inst|
    (Euclidean norms; M bounds every coordinate of every intermediate point, rotations keeping norms).  Derivation, u = 2^-53:
      * one output coordinate of a transform, fl(R_i . x + t_i), is three products and three additions; in whatever order, fused
        or not, its error is at most 4 u (|R_i| . |x| + |t_i|) <= 4 u (|x|_2 + |t|_2) <= 8 u M (a rotation's row has norm 1);
      * so two correct implementations (numpy's einsum and the kernel) differ by at most 16 u M per coordinate after the ego
        transform, sqrt(3) 16 u M as a vector, and the instance transform carries that into at most sqrt(3) 16 u M per
        coordinate and adds its own 16 u M: (1 + sqrt 3) 16 u M < 44 u M;
      * the subtraction p_full - p rounds once in each implementation: 2 . u . 2 M = 4 u M.
    48 u M in all; 64 leaves room for poses whose rotation rows are unit only to rounding.  For these fixtures M is about
    60 m: 4e-13 m."""
    from icp_flow_amd import utils_loading
    g = sr.load(name)
    raw, t, inst, ego, tsfm = g["raw_points"], g["time_indice"], g["inst_labels"], g["ego_motion_gt"], g["bbox_tsfm"]
    got = utils_loading.scene_flow(raw, t, inst, ego, tsfm)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == g["scene_flow"].shape
    bound = sr.gt_flow_bound(raw, ego, tsfm)
    err = np.abs(got - g["scene_flow"]).max()
    print(f"{name}: max |scene_flow - reference| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(got - sr.gt_flow_numpy(raw, t, inst, ego, tsfm)).max() <= bound
    # the two functions of the reference, one step each: the same arithmetic, so the same bits; device tensors stay on the device
    F = int(g["num_frames"])
    step = utils_loading.reconstruct_sequence(utils_loading.ego_motion_compensation(raw, t, ego), t, inst, tsfm, F)
    assert np.array_equal(step - raw, got)
    on_dev = utils_loading.reconstruct_sequence(utils_loading.ego_motion_compensation(G(raw), G(t), G(ego)), G(t), G(inst), G(tsfm), F)
    assert isinstance(on_dev, torch.Tensor) and on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), step)


def _epe_bound(sf_bound):
    # the issue's bound: any summation order against numpy's pairwise one, 2 n 2^-53 relative, plus the ground truth's own bound
    return lambda value, n: 2 * n * sr.U * value + sf_bound


@pytest.mark.parametrize("eg", [0, 1], ids=["crop", "eval_ground"])
@pytest.mark.parametrize("name", FIXTURES)
def test_table_against_g13(name, eg):
    """calculate_metrics on the fixture's sample: every count exactly the reference's (recovered as round(fraction * n) from its
    float32 fractions and weights), every mean error within 2 n 2^-53 relative + the scene-flow bound, and all 6 x (F + 1) meters
    -- num, weights, *_data, *_avg, fractions equal as float32 -- as the reference's calculate_metrics left them."""
    from icp_flow_amd import utils_eval
    g = sr.load(name)
    args, data, pred = sr.crop_args(g, eg), sr.sample(g), g["pred_flow"]
    sf_bound = sr.gt_flow_bound(g["raw_points"], g["ego_motion_gt"], g["bbox_tsfm"])
    table, esum, kept0, outside = utils_eval.sequence_table(args, data, pred)
    want, want_epe, want_kept0 = sr.reference_table(g, eg)
    counts = table.copy()
    counts[:, :, 1] = 0
    assert np.array_equal(counts, want) and kept0 == want_kept0 and outside == 0
    F = args.num_frames
    for j in range(F):
        for c in range(6):
            n = int(table[j, c, 0])
            if n and not np.isnan(want_epe[j, c]):
                got = esum[j, c] / n
                print(f"{name} eg{eg} row {j} class {c}: n {n}, mean e {got!r} vs {want_epe[j, c]!r}")
                assert abs(got - want_epe[j, c]) <= _epe_bound(sf_bound)(want_epe[j, c], n)
    meters = utils_eval.calculate_metrics(args, data, pred, utils_eval.new_metric_table(F))
    sr.check_meters(meters, g, eg, _epe_bound(sf_bound))
    # ... and with the ground truth the GPU builds itself instead of the fixture's
    from icp_flow_amd import utils_loading
    data2 = dict(data, scene_flow=utils_loading.scene_flow(g["raw_points"], g["time_indice"], g["inst_labels"], g["ego_motion_gt"], g["bbox_tsfm"]))
    meters2 = utils_eval.calculate_metrics(args, data2, pred, utils_eval.new_metric_table(F))
    sr.check_meters(meters2, g, eg, _epe_bound(sf_bound))


@pytest.mark.parametrize("eg", [0, 1], ids=["crop", "eval_ground"])
@pytest.mark.parametrize("prefix", ["no_dynamic_fg__", "no_static__"])
def test_empty_classes_as_the_reference(prefix, eg):
    """A sequence without a dynamic_fg point: those rows are skipped (utils_eval.py:254).  A sequence without a static point:
    `static_j` is updated all the same, with NaN and weight 0 (utils_eval.py:217-222).  Both as the reference's code left its
    meters on the same input."""
    from icp_flow_amd import utils_eval
    g = sr.load("g13_seqeval_edge")
    args, data = sr.crop_args(g, eg, prefix), sr.sample(g, prefix)
    meters = utils_eval.calculate_metrics(args, data, g[prefix + "pred_flow"], utils_eval.new_metric_table(args.num_frames))
    sr.check_meters(meters, g, eg, _epe_bound(0.0), prefix)
    if prefix == "no_static__":
        assert np.isnan(meters["static_1"].epe_avg) and meters["static_1"].num_data == [0]
    else:
        assert meters["dynamic_fg_1"].num_data == [] and meters["dynamic_fg_0"].num == 0


def _random_sample(m, F, seed):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(-40, 40, size=(m, 3))
    raw[:, 2] = rng.uniform(-0.5, 2.0, size=m)
    gt = rng.normal(size=(m, 3)) * rng.uniform(0.0, 1.5, size=(m, 1))
    pred = (gt + rng.normal(size=(m, 3)) * rng.uniform(0.0, 0.4, size=(m, 1))).astype(np.float32)
    # (unsorted time indices: a tile of 64 rows holds several gaps; labels outside {0, 1} count in `overall` only)
    data = dict(raw_points=raw, time_indice=rng.integers(0, F, size=m), sd_labels=rng.choice([0, 1, 1, 0, -1], size=m),
                fb_labels=rng.choice([0, 1, 2], size=m), scene_flow=gt)
    return data, pred


# one workgroup is sized for 256 threads x 8 rows = 2048 rows (csrc/seqeval.hip); 3 * 2048 + 777: several workgroups and a ragged tail;
# 600000: more rows than the 256 workgroups of the largest grid take in one round
@pytest.mark.parametrize("F", [2, 16])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 777, 600000])
def test_shapes_where_the_reduction_can_go_wrong(m, F):
    from icp_flow_amd import utils_eval
    data, pred = _random_sample(m, F, seed=1000 * F + m)
    for eg in (0, 1):
        args = SimpleNamespace(num_frames=F, eval_ground=bool(eg), range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
        table, esum, kept0, outside = utils_eval.sequence_table(args, data, pred)
        want, want_sum, want_kept0 = sr.table_numpy(args, data, pred)
        counts = table.copy()
        counts[:, :, 1] = 0
        assert np.array_equal(counts, want) and kept0 == want_kept0 and outside == 0
        assert np.array_equal(table[0, :, 0], table[1:, :, 0].sum(axis=0))
        n = np.maximum(want[:, :, 0], 1)
        assert (np.abs(esum - want_sum) <= 2 * n * sr.U * np.abs(want_sum)).all(), np.abs(esum - want_sum).max()


def test_determinism_across_runs_and_streams():
    """Two runs, and a run on a second stream, give a bit-identical table (the sums of e included)."""
    from icp_flow_amd import _lib
    F, m = 5, 5 * 2048 + 333
    data, pred = _random_sample(m, F, seed=77)
    pts, tim = G(data["raw_points"]), G(data["time_indice"].astype(np.int32))
    sd, fb = G(data["sd_labels"].astype(np.int32)), G(data["fb_labels"].astype(np.int32))
    gt, pr = G(data["scene_flow"]), G(pred)
    need = _lib._L.icpflow_seq_metrics_workspace_bytes(m, F)

    def run(stream):
        out = torch.full((F * 36 + 2,), -1, dtype=torch.int64, device=DEV)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        with torch.cuda.stream(stream):
            _lib.call("icpflow_seq_metrics", _lib.ptr(pts), _lib.ptr(tim), _lib.ptr(sd), _lib.ptr(fb), _lib.ptr(gt), _lib.ptr(pr), m, F,
                      _lib.SEQ_CROP_XYZ, 32.0, 32.0, 0.3, _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + F * 36 * 8), _lib.ptr(ws),
                      ctypes.c_size_t(need), _lib.stream(DEV))
        stream.synchronize()
        return out.cpu()

    torch.cuda.synchronize()
    first = run(torch.cuda.current_stream(DEV))
    assert torch.equal(run(torch.cuda.current_stream(DEV)), first)
    assert torch.equal(run(torch.cuda.Stream(DEV)), first)
    assert int(first[36]) > 0


def test_out_of_range_rows_are_reported_and_not_written():
    from icp_flow_amd import _lib, utils_eval, utils_loading
    g = sr.load("g13_seqeval_edge")
    p = "no_static__"
    raw, t, inst = g[p + "raw_points"], g[p + "time_indice"].copy(), g[p + "inst_labels"].copy()
    ego, tsfm = g[p + "ego_motion_gt"], g[p + "bbox_tsfm"]
    F, K, m = tsfm.shape[1], tsfm.shape[0], len(raw)
    bad_rows = np.array([0, 5, 64, 65, m - 1])
    t[bad_rows[0]], t[bad_rows[1]] = -1, F              # (numpy would wrap -1 around to the last frame)
    inst[bad_rows[2]], inst[bad_rows[3]], inst[bad_rows[4]] = -1, K, 1 << 20
    GUARD = 777.25
    out = torch.full((m, 3), GUARD, dtype=torch.float64, device=DEV)
    bad = torch.full((1,), -5, dtype=torch.int64, device=DEV)
    need = _lib._L.icpflow_seq_gt_flow_workspace_bytes(m)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    keep = [G(raw.astype(np.float64)), G(t.astype(np.int32)), G(inst.astype(np.int32)), G(ego), G(tsfm)]
    _lib.call("icpflow_seq_gt_flow", _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]), m, _lib.ptr(keep[3]), F, _lib.ptr(keep[4]), K,
              _lib.SEQ_OUT_FLOW, _lib.ptr(out), _lib.ptr(bad), _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert int(bad.item()) == len(bad_rows)
    assert (got[bad_rows] == GUARD).all()
    good = np.setdiff1d(np.arange(m), bad_rows)
    assert np.array_equal(got[good], utils_loading.scene_flow(raw[good], t[good], inst[good], ego, tsfm)) and not (got[good] == GUARD).any()
    with pytest.raises(IndexError, match="5 of"):
        utils_loading.scene_flow(raw, t, inst, ego, tsfm)
    with pytest.raises(IndexError, match="time index"):
        utils_loading.ego_motion_compensation(raw, t, ego)
    # the table: a time index outside [0, F) is counted apart and nowhere else
    args, data = sr.crop_args(g, 1, p), dict(sr.sample(g, p), time_indice=t)
    table, _, _, outside = utils_eval.sequence_table(args, data, g[p + "pred_flow"])
    assert outside == 2 and table[0, 0, 0] == int(((t >= 1) & (t < F)).sum())
    with pytest.raises(ValueError, match="outside"):
        utils_eval.calculate_metrics(args, data, g[p + "pred_flow"], utils_eval.new_metric_table(F))


def test_cpu_tensors_are_refused_with_a_gpu_present():
    from icp_flow_amd import utils_eval, utils_loading
    g = sr.load("g13_seqeval_edge")
    p = "no_static__"
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_loading.reconstruct_sequence(T(g[p + "raw_points"]), T(g[p + "time_indice"]), T(g[p + "inst_labels"]), T(g[p + "bbox_tsfm"]), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.calculate_metrics(sr.crop_args(g, 0, p), {k: T(v) for k, v in sr.sample(g, p).items()}, T(g[p + "pred_flow"]),
                                     utils_eval.new_metric_table(3))


def test_a_device_flow_crosses_to_the_host_as_the_table_only(monkeypatch):
    """calculate_metrics with device tensors: the one device -> host copy is the table (F * 36 + 2 words); no input is brought
    to the host (no .cpu(), .numpy(), .item() or .tolist() on anything else)."""
    from icp_flow_amd import utils_eval
    g = sr.load("g13_seqeval_f3_f32")
    args = sr.crop_args(g, 0)
    data = {k: G(v) for k, v in sr.sample(g).items()}
    pred = G(g["pred_flow"])
    copies, others = [], []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.numel()), real_cpu(self, *a, **k))[1])
    for name in ("item", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda real, name: lambda self, *a, **k: (others.append(name) if self.is_cuda else None,
                                                                                          real(self, *a, **k))[1])(real, name))
    meters = utils_eval.calculate_metrics(args, data, pred, utils_eval.new_metric_table(3))
    monkeypatch.undo()
    assert copies == [3 * 36 + 2] and others == []
    sr.check_meters(meters, g, 0, _epe_bound(0.0))


def test_run_sequences_end_to_end(tmp_path):
    """An F = 3 synthetic sample through run_sequences: its table equals calculate_metrics applied to the flows the existing
    path (load_sequence + register_frame_pair, what run_stream does) returns for the same frame pairs, brought to the host and
    stacked as main.py:217-260 does -- counts equal, mean errors within the summation bound."""
    from icp_flow_amd import frame_pairs, synthetic, utils_eval
    d = synthetic.make_sequence(seed=3, num_frames=3, n_objects=6, n_max=400)
    rng = np.random.default_rng(4)
    m = len(d["raw_points"])
    sd = (d["nonground"] & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    os.makedirs(os.path.join(tmp_path, "val"))
    path = os.path.join(tmp_path, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=d["nonground"].astype(np.int64))
    a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.05, False, "ego_motion_gt"
    res = frame_pairs.run_sequences(a, [path], DEV)
    assert res["sequences"] == 1 and res["frame_pairs"] == 2 and res["ground"] == "nonground key" and res["ms_per_sequence"] > 0
    sample = frame_pairs.load_sequence_sample(path, a)
    assert sample["scene_flow"].dtype == np.float64 and len(sample["raw_points"]) == m
    flows = np.zeros((m, 3), np.float32)
    for fp in frame_pairs.load_sequence(path, a):
        flows[sample["time_indice"] == fp.gap] = frame_pairs.register_frame_pair(a, fp, DEV)["flow"].cpu().numpy()
    want = utils_eval.calculate_metrics(a, sample, flows, utils_eval.new_metric_table(3))
    table, esum, kept0 = sr.table_numpy(a, sample, flows)
    by_numpy = utils_eval.update_meters(a, utils_eval.new_metric_table(3), table, esum, kept0)
    assert table[0, 4, 0] > 0 and table[0, 1, 0] > 0          # dynamic and static points are evaluated
    for name, got in res["metrics"].items():
        for ref in (want[name], by_numpy[name]):
            assert got.num == ref.num and got.num_data == ref.num_data, name
            for metric in sr.METRICS[1:]:
                assert sr.same_f32(getattr(got, metric + "_avg"), getattr(ref, metric + "_avg")), (name, metric)
            n = max(float(table[0, 0, 0]), 1.0)
            assert abs(got.epe_avg - ref.epe_avg) <= 2 * n * sr.U * abs(ref.epe_avg) or (np.isnan(got.epe_avg) and np.isnan(ref.epe_avg)), name
    assert res["metrics"]["overall_0"].epe_avg < 0.5
    text = utils_eval.format_metric_table(res["metrics"], 3)
    assert text.count("\n") == 6 * 4

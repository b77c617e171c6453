"""CPU-only part of the sequence evaluation (icpflow_seq_gt_flow / icpflow_seq_metrics, utils_loading, utils_eval.calculate_metrics,
frame_pairs.run_sequences): the ABI, argument errors, the refusal of CPU tensors, the g13 fixtures' margin condition, the host
half of calculate_metrics (table -> the reference's meters) on a numpy-made table, and that what existed is unchanged."""
import ctypes
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seqeval_restatement as sr      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["icpflow_seq_gt_flow", "icpflow_seq_gt_flow_workspace_bytes", "icpflow_seq_metrics", "icpflow_seq_metrics_workspace_bytes"]
FIXTURES = ["g13_seqeval_f3_f32", "g13_seqeval_f3_f64", "g13_seqeval_f5_f32", "g13_seqeval_f5_f64"]
EDGE = ["no_dynamic_fg__", "no_static__"]


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as entry
    from icp_flow_amd import _lib
    lib = ctypes.CDLL(entry.build())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "icpflow_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES, f"{name} not bound"
    assert "#define ICPFLOW_SEQ_MAX_FRAMES 16" in hdr and _lib.SEQ_MAX_FRAMES == 16
    assert (_lib.SEQ_OUT_FLOW, _lib.SEQ_OUT_POINTS, _lib.SEQ_CROP_NONE, _lib.SEQ_CROP_XY, _lib.SEQ_CROP_XYZ) == (0, 1, 0, 1, 2)
    # a partial of a workgroup: (F - 1) * 36 + 2 words; a workgroup per 2048 rows, 256 at most; multiples of 256 bytes
    ws = lib.icpflow_seq_metrics_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert ws(0, 2) == 512 and ws(2048, 2) == 512 and ws(2049, 2) == 768 and ws(1 << 30, 16) == 256 * (15 * 36 + 2) * 8
    assert ws(10, 17) == 0 and ws(-1, 3) == 0
    sizes = [ws(m, 5) for m in (0, 1, 2048, 2049, 100000, 524288, 524289, 1 << 24)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)


def test_argument_errors_are_status_codes_with_messages():
    from icp_flow_amd import _lib
    L, one = _lib._L, ctypes.c_void_p(64)
    big = ctypes.c_size_t(1 << 30)
    metrics = lambda m, F, ws=one, nbytes=big, crop=2, pts=one, table=one: L.icpflow_seq_metrics(   # noqa: E731
        pts, one, one, one, one, one, m, F, crop, 32.0, 32.0, 0.3, table, one, ws, nbytes, None)
    assert metrics(10, 17) == -3 and b"F = 17" in L.icpflow_last_error()
    assert metrics(-1, 3) == -1 and b"m < 0" in L.icpflow_last_error()
    assert metrics(10, 0) == -1 and b"F must be" in L.icpflow_last_error()
    assert metrics(10, 3, crop=5) == -1 and b"crop" in L.icpflow_last_error()
    assert metrics(10, 3, pts=None) == -1 and b"null pointer" in L.icpflow_last_error()
    assert metrics(10, 3, table=None) == -1 and b"null pointer" in L.icpflow_last_error()
    assert metrics(10, 3, ws=None) == -2 and b"workspace" in L.icpflow_last_error()
    need = L.icpflow_seq_metrics_workspace_bytes(5000, 3)
    assert metrics(5000, 3, nbytes=ctypes.c_size_t(need - 1)) == -2 and str(need).encode() in L.icpflow_last_error()
    flow = lambda m, F=3, K=2, out=0, ws=one, nbytes=big, ego=one, tsfm=one, inst=one, bad=one: L.icpflow_seq_gt_flow(   # noqa: E731
        one, one, inst, m, ego, F, tsfm, K, out, one, bad, ws, nbytes, None)
    assert flow(-1) == -1 and b"m < 0" in L.icpflow_last_error()
    assert flow(10, F=0) == -1 and b"F must be" in L.icpflow_last_error()
    assert flow(10, out=7) == -1 and b"output" in L.icpflow_last_error()
    assert flow(10, bad=None) == -1 and b"null pointer" in L.icpflow_last_error()
    assert flow(10, ego=None, tsfm=None) == -1 and b"null pointer" in L.icpflow_last_error()
    assert flow(10, inst=None) == -1 and b"null pointer" in L.icpflow_last_error()
    assert flow(10, ws=None) == -2 and b"workspace" in L.icpflow_last_error()
    need = L.icpflow_seq_gt_flow_workspace_bytes(10)
    assert need == 256 and flow(10, nbytes=ctypes.c_size_t(need - 1)) == -2 and b"workspace" in L.icpflow_last_error()


def test_numpy_input_without_a_gpu_is_refused(monkeypatch):
    """numpy input is uploaded when there is a GPU; without one it is refused like a CPU tensor (no CPU path)"""
    from icp_flow_amd import utils_eval, utils_loading
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    g = sr.load("g13_seqeval_edge")
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_loading.reconstruct_sequence(g["no_static__raw_points"], g["no_static__time_indice"], g["no_static__inst_labels"],
                                           g["no_static__bbox_tsfm"], 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.calculate_metrics(sr.crop_args(g, 0, "no_static__"), sr.sample(g, "no_static__"), g["no_static__pred_flow"],
                                     utils_eval.new_metric_table(3))


def test_cpu_tensors_are_refused():
    from icp_flow_amd import utils_eval, utils_loading
    g = sr.load("g13_seqeval_edge")
    p = "no_static__"
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_loading.reconstruct_sequence(T(g[p + "raw_points"]), T(g[p + "time_indice"]), T(g[p + "inst_labels"]), T(g[p + "bbox_tsfm"]), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_loading.ego_motion_compensation(T(g[p + "raw_points"]), T(g[p + "time_indice"]), T(g[p + "ego_motion_gt"]))
    data = {k: T(v) for k, v in sr.sample(g, p).items()}
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.calculate_metrics(sr.crop_args(g, 0, p), data, T(g[p + "pred_flow"]), utils_eval.new_metric_table(3))


def _cases():
    for name in FIXTURES:
        yield name, ""
    for p in EDGE:
        yield "g13_seqeval_edge", p


@pytest.mark.parametrize("name,prefix", list(_cases()))
def test_fixture_margin_condition(name, prefix):
    """tools/gen_golden_seqeval.py's MARGIN CONDITION from the stored reference values: no e or r within 1e-9 (relative) of a
    predicate threshold, no coordinate within 1e-9 of a crop bound (the bound as given and as float32) -- a last-bit difference
    cannot move a point across, so the GPU's counts must equal the reference's exactly."""
    g = sr.load(name)
    e, r = sr.errors(g[prefix + "scene_flow"], g[prefix + "pred_flow"])
    for thr in (0.05, 0.1, 0.3):
        assert (np.abs(e - thr) > 1e-9 * thr).all() and (np.abs(r - thr) > 1e-9 * thr).all()
        assert 0 < (e < thr).sum() < len(e)                      # members on both sides
    raw = g[prefix + "raw_points"].astype(np.float64)
    a = sr.crop_args(g, 0, prefix)
    for col, bound in ((np.abs(raw[:, 0]), a.range_x), (np.abs(raw[:, 1]), a.range_y), (raw[:, 2], a.range_z + a.ground_slack)):
        for b in (bound, float(np.float32(bound))):
            assert (np.abs(col - b) > 1e-9 * abs(b)).all()
        if not prefix or bound < 1.0:                            # (the small edge samples lie inside the crop in x and y)
            assert 0 < (col < bound).sum() < len(col)            # points outside the crop / below z_min exist
    assert g[prefix + "scene_flow"].dtype == np.float64 and g[prefix + "pred_flow"].dtype == np.float32
    assert (g[prefix + "pred_flow"][g[prefix + "time_indice"] == 0] == 0).all()


@pytest.mark.parametrize("eg", [0, 1])
@pytest.mark.parametrize("name,prefix", list(_cases()))
def test_meters_from_a_numpy_table_equal_the_reference(name, prefix, eg):
    """The host half of calculate_metrics (table -> meter updates, the reference's quirks included) fed with the numpy
    restatement of the kernel's table: every meter as the reference left it.  The edge cases carry an empty `dynamic_fg` class
    (rows skipped, utils_eval.py:254) and an empty `static` class (updated with NaN and weight 0, utils_eval.py:217-222)."""
    from icp_flow_amd import utils_eval
    g = sr.load(name)
    args, data = sr.crop_args(g, eg, prefix), sr.sample(g, prefix)
    table, esum, kept0 = sr.table_numpy(args, data, g[prefix + "pred_flow"])
    want, _, want_kept0 = sr.reference_table(g, eg, prefix)
    assert np.array_equal(table, want) and kept0 == want_kept0
    meters = utils_eval.new_metric_table(args.num_frames)
    assert list(meters) == utils_eval.metric_table_names(args.num_frames)
    utils_eval.update_meters(args, meters, table, esum, kept0)
    sr.check_meters(meters, g, eg, lambda v, n: 2 * n * sr.U * v, prefix)
    if prefix == "no_static__":
        assert np.isnan(meters["static_1"].epe_avg) and meters["static_1"].num == 0 and meters["static_bg_1"].num_data == []
    if prefix == "no_dynamic_fg__":
        assert meters["dynamic_fg_0"].num_data == [] and meters["dynamic_1"].num > 0
    text = utils_eval.format_metric_table(meters, args.num_frames)
    lines = text.split("\n")
    assert len(lines) == 1 + 6 * (args.num_frames + 1) and lines[0].startswith("################# Results over the entire dataset")
    assert lines[1].startswith("overall_0   , EPE3D: ") and ",                   ACC3DS: " in lines[1] and lines[1].endswith(".")


def test_what_existed_is_unchanged(tmp_path):
    """load_sequence and run_stream on a sequence sample: the arrays and the summary they gave before the sequence evaluation
    was added (pinned as a digest and as numbers; the register function is a stand-in, there is no GPU here)."""
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_sequence(seed=5, num_frames=3, n_objects=4, n_max=120, n_background=150)
    os.makedirs(os.path.join(tmp_path, "val"))
    path = os.path.join(tmp_path, "val", "s0.npz")
    np.savez(path, **d)
    a = frame_pairs.default_args(speed=0.8333, range_x=30.0, range_y=30.0)
    fps = frame_pairs.load_sequence(path, a, pose_source="ego_motion_gt")
    h = hashlib.sha256()
    for fp in fps:
        for k in ("points_src", "points_dst", "points_src_raw", "pose", "pose_exact", "gt_flow", "nonground_src", "nonground_dst"):
            h.update(np.ascontiguousarray(getattr(fp, k)).tobytes())
        h.update(f"{fp.gap}|{fp.name}|{fp.pose_source}".encode())
    assert h.hexdigest() == PINNED_DIGEST

    def register(args, fp, device):
        flow = torch.from_numpy(fp.gt_flow + np.float32(0.04) * fp.gap)
        return dict(pairs=torch.zeros((fp.gap, 10)), transformations=torch.zeros((fp.gap, 4, 4)), flow=flow)

    a.pose_source = "ego_motion_gt"
    s = frame_pairs.run_stream(a, [path], "cpu", register_fn=register)
    timing = {k: s.pop(k) for k in ("ms_per_frame_pair", "frame_pairs_per_s")}
    assert all(v > 0 for v in timing.values())
    assert s == PINNED_SUMMARY
    assert sorted(frame_pairs.DEFAULT_ARGS) == PINNED_DEFAULT_ARGS


PINNED_DIGEST = '27c3b827d7ebe6c46f979b8b7d928ae20a4b2473ef73790a0b2021ead013208a'
PINNED_SUMMARY = {'frame_pairs': 2, 'matched_cluster_pairs': 3, 'n_gpus': 1, 'evaluated_points': 999, 'pose_sources': {'ego_motion_gt': 2}, 'epe': 0.10388834268839152, 'accs': 0.7387387387387387, 'accr': 0.9179179179179179, 'outlier': 0.15715715715715717, 'Routlier': 0.0}
PINNED_DEFAULT_ARGS = ['chunk_size', 'cluster', 'epsilon', 'max_points', 'min_cluster_size', 'native_host', 'num_clusters', 'range_x', 'range_y', 'speed', 'thres_box', 'thres_dist', 'thres_error', 'thres_iou', 'thres_rot', 'tight_padding', 'translation_frame']

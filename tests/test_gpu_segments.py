"""The per-segment evaluation on the GPU (icpflow_seq_segment_table, utils_flow.flow_evaluation, utils_debug.debug_frame,
run_sequences with if_verbose) against the g14 fixtures -- the reference's own verbose loop run on the CPU,
tools/gen_golden_segments.py -- and against the numpy restatement (tests/segment_restatement.py) on the shapes where the
reduction can go wrong.  Segments are cut into chunks of C = 1024 rows (csrc/segeval.hip); the sizes below are built around it."""
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
import segment_restatement as sg      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = sg.CHUNK
G = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
SENTINEL = -777.25


def raw_table(pts, labels, pred=None, gt=None, z_min=-np.inf, Lmax=64, stream=None):
    """the entry point itself -> (table [Lmax,16] numpy, prefilled with a sentinel, num)"""
    from icp_flow_amd import _lib
    n = len(labels)
    keep = [G(np.asarray(pts, np.float64).reshape(-1, 3)), G(np.asarray(labels, np.float32)), G(None if gt is None else np.asarray(gt, np.float64)),
            G(None if pred is None else np.asarray(pred, np.float32))]
    need = _lib._L.icpflow_seq_segment_table_workspace_bytes(n, Lmax)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=DEV)
    table = torch.full((Lmax, 16), SENTINEL, dtype=torch.float64, device=DEV)
    num = torch.full((1,), -12345, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    with torch.cuda.stream(st):
        _lib.call("icpflow_seq_segment_table", _lib.ptr(keep[0]), _lib.ptr(keep[1]), n, _lib.ptr(keep[2]), _lib.ptr(keep[3]), float(z_min),
                  _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    st.synchronize()
    return table.cpu().numpy(), int(num.item())


def against_restatement(pts, labels, pred, gt, z_min, Lmax=64):
    want, _, absx, absm = sg.table_numpy(pts, labels, pred, gt, z_min)
    got, num = raw_table(pts, labels, pred, gt, sg.z_threshold(z_min, pts), Lmax)
    assert num == len(want)
    sg.check_table(got[:num], want, absx, absm, flows=gt is not None)
    assert (got[num:] == SENTINEL).all()                     # rows from num on are not written
    return got[:num], want


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "all"])
@pytest.mark.parametrize("name", sg.FIXTURES)
def test_table_and_report_against_g14(name, crop):
    """Counts equal to the reference's; the sum of e per segment within (n - 1) 2^-53 sum e of math.fsum of the restatement's per-row e,
    the coordinate sums within the same bound with sum |x|; the Python report equal to the fixture as check_report compares
    (fractions equal as float32, EPE and means within the bound of two summation orders); the printed lines the reference's."""
    from icp_flow_amd import utils_flow
    g = sg.load(name)
    z_min = float(g["z_min"]) if crop else None
    tag = "crop_" if crop else "all_"
    want, e, absx, absm = sg.table_numpy(g["src_points"], g["src_labels"], g["flow_pd"], g["flow_gt"], z_min)
    table, num = utils_flow.segment_table(G(g["src_points"]), G(g["src_labels"]), G(g["flow_pd"]), G(g["flow_gt"]), z_min=z_min)
    assert num == len(want) == 14 and table.is_cuda and table.shape == (14, 16)
    got = table.cpu().numpy()
    for c in range(num):
        print(f"{name} {tag} segment {got[c, 0]:.0f}: kept {got[c, 2]:.0f}, sum e {got[c, 3]!r} vs fsum {want[c, 3]!r}")
    sg.check_table(got, want, absx, absm)
    has = got[:, 2] > 0
    assert np.array_equal(got[has, 0].astype(np.int64), g[tag + "labels"]) and np.array_equal(got[has, 2].astype(np.int64), g[tag + "len_i"])
    for k, col in (("accs", 4), ("accr", 5), ("outlier", 6), ("routlier", 7)):     # every predicate count the reference's
        assert np.array_equal(got[has, col], np.round(g[tag + k].astype(np.float64) * g[tag + "len_i"])), k
    dwant, _, dabsx, dabsm = sg.table_numpy(g["dst_points"], g["dst_labels"])
    dtab, dnum = utils_flow.segment_table(G(g["dst_points"]), G(g["dst_labels"]))
    sg.check_table(dtab.cpu().numpy(), dwant, dabsx, dabsm, flows=False)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rep = utils_flow.flow_evaluation(G(g["src_points"]), G(g["dst_points"]), G(g["src_labels"]), G(g["dst_labels"]), G(g["flow_pd"]),
                                         G(g["flow_gt"]), G(g["pose"]), G(g["transformations"]), pairs=G(g["pairs"]), z_min=z_min, verbose=True)
    sg.check_report(rep, g, crop)
    sg.check_lines(rep.lines, g, crop)
    assert out.getvalue() == "".join(x + "\n" for x in rep.lines)
    if crop:
        k = int(np.flatnonzero(rep.label == 23)[0])
        assert rep.n[k] == 0 and rep.rows[k] > 0 and np.isnan(rep.epe[k]) and np.isnan(rep.translation[k])


@pytest.mark.parametrize("name", sg.FIXTURES)
def test_debug_frame_against_g14(name):
    """The three per-frame rows through icpflow_seq_metrics: counts and float32 fractions the reference's, EPE within the bound
    of two summation orders, the printed lines equal; under if_verbose the segments as well."""
    from icp_flow_amd import utils_debug
    g = sg.load(name)
    for eval_ground, tag in ((False, "crop_"), (True, "all_")):
        args = SimpleNamespace(num_frames=2, eval_ground=eval_ground, range_z=float(g["range_z"]), ground_slack=float(g["ground_slack"]),
                               if_verbose=not eval_ground)
        result = dict(j=1, src=G(g["src_points"]), dst=G(g["dst_points"]), pose=G(g["pose"]), sd_label=G(g["sd_label"]), fb_label=G(g["fb_label"]),
                      scene_flow=G(g["flow_gt"]), src_label=G(g["src_labels"]), dst_label=G(g["dst_labels"]), flow=G(g["flow_pd"]),
                      transformations=G(g["transformations"]), pairs=G(g["pairs"]))
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            got = utils_debug.debug_frame(args, result)
        want = g[tag + "frame_rows"]
        for k, row in zip(utils_debug.FRAME_CLASSES, want):
            v = got["frame"][k]
            assert v[5] == int(row[5]) and all(sg.same_f32(a, b) for a, b in zip(v[1:5], row[1:5])), k
            assert abs(v[0] - row[0]) <= sg.mean_bound(row[5], row[0], np.float64), k
        assert got["lines"] == str(g[tag + "frame_text"]).strip().split("\n")
        assert out.getvalue().startswith("".join(x + "\n" for x in got["lines"]))
        if eval_ground:
            assert got["segments"] is None
        else:
            sg.check_report(got["segments"], g, True)
            sg.check_lines(got["segments"].lines, g, True)


SIZES = [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 777]
IDS = [-1e8, -1, 0, 5, 199, 4000, 7, 8, 9, 10, 11]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_shapes_where_the_reduction_can_go_wrong(dtype):
    """Segments of 1 .. 3 C + 777 rows in one cloud, rows interleaved; ids 0, 5, 199, 4000 beside -1 and -1e8; one segment with
    every row cropped; with the crop, without, and in the no-flow form."""
    labels = sg.interleaved_labels(SIZES, IDS, seed=5)
    pts, gt, pred = sg.random_cloud(labels, seed=6, dtype=dtype)
    pts[labels == 199, 2] = -1.0                              # every row of segment 199 below z_min
    for z_min in (0.3, None):
        got, want = against_restatement(pts, labels, pred, gt, z_min)
        assert list(got[:, 0]) == sorted(np.float32(IDS).astype(float)) and sorted(got[:, 1]) == sorted(SIZES)
        if z_min is not None:
            k = list(got[:, 0]).index(199.0)
            assert got[k, 1] == 255 and (got[k, 2:] == 0).all()
            assert 0 < got[:, 2].sum() < len(labels)
        against_restatement(pts, labels, None, None, z_min)


def test_both_zeros_are_one_segment():
    """-0.0 and +0.0 are one label (table.hip's label_key, whose dictionary and order the segments reuse; np.unique in the
    restatement): one segment of all their rows, reported as 0.0"""
    labels = sg.interleaved_labels([300, 200, 100], [0.0, -0.0, 5.0], seed=9)
    pts, gt, pred = sg.random_cloud(labels, seed=10)
    got, _ = against_restatement(pts, labels, pred, gt, None)
    assert got.shape[0] == 2 and got[0, 1] == 500 and got[0, 0] == 0 and not np.signbit(got[0, 0])


def test_single_segment_lmax_exact_overflow_and_empty():
    from icp_flow_amd import _lib
    # one segment covering the whole cloud: 2 C + 100 rows, three chunks
    labels = np.full(2 * C + 100, 3.0, np.float32)
    pts, gt, pred = sg.random_cloud(labels, seed=8)
    got, _ = against_restatement(pts, labels, pred, gt, 0.3, Lmax=1)
    assert got.shape == (1, 16) and got[0, 1] == 2 * C + 100
    # Lmax distinct labels exactly, then one more
    for Lmax in (37, 4096):
        ids = np.arange(Lmax) * 3 - 50
        labels = sg.interleaved_labels([2] * Lmax, ids, seed=Lmax)
        pts, gt, pred = sg.random_cloud(labels, seed=Lmax + 1)
        got, _ = against_restatement(pts, labels, pred, gt, None, Lmax=Lmax)
        assert len(got) == Lmax and (got[:, 1] == 2).all()
        labels = np.concatenate([labels, np.float32([1e6])])
        pts, gt, pred = sg.random_cloud(labels, seed=Lmax + 2)
        table, num = raw_table(pts, labels, pred, gt, Lmax=Lmax)
        assert num == -(Lmax + 1) and (table == SENTINEL).all()
    # n = 0
    table, num = raw_table(np.zeros((0, 3)), np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3)))
    assert num == 0 and (table == SENTINEL).all()
    from icp_flow_amd import utils_flow
    with pytest.raises(RuntimeError, match="distinct labels"):
        utils_flow.segment_table(G(pts), G(labels), max_segments=64)
    assert _lib.VERSION == 215


def test_determinism_across_runs_and_streams():
    """Three reruns give bit-identical tables; two calls in flight on two streams at once, each on its own workspace, too."""
    from icp_flow_amd import _lib
    labels = sg.interleaved_labels(SIZES, IDS, seed=15)
    pts, gt, pred = sg.random_cloud(labels, seed=16)
    first, num = raw_table(pts, labels, pred, gt, 0.3)
    assert num == len(IDS)
    for _ in range(2):
        again, _ = raw_table(pts, labels, pred, gt, 0.3)
        assert again.tobytes() == first.tobytes()
    n, Lmax = len(labels), 64
    dev = [G(pts), G(labels), G(gt), G(pred)]
    need = _lib._L.icpflow_seq_segment_table_workspace_bytes(n, Lmax)
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    outs = [(torch.full((Lmax, 16), SENTINEL, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
             torch.empty(need, dtype=torch.uint8, device=DEV)) for _ in streams]
    torch.cuda.synchronize()
    for _ in range(3):                                          # enqueued alternately: the two chains overlap on the device
        for st, (table, num_t, ws) in zip(streams, outs):
            with torch.cuda.stream(st):
                _lib.call("icpflow_seq_segment_table", _lib.ptr(dev[0]), _lib.ptr(dev[1]), n, _lib.ptr(dev[2]), _lib.ptr(dev[3]), 0.3,
                          _lib.ptr(table), Lmax, _lib.ptr(num_t), _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(DEV))
    torch.cuda.synchronize()
    for table, num_t, _ in outs:
        assert int(num_t.item()) == num and table.cpu().numpy().tobytes() == first.tobytes()


@pytest.fixture(scope="module")
def sequence_runs(tmp_path_factory):
    """one synthetic F = 3 sequence through run_sequences without and with if_verbose (shared by the tests below)"""
    from icp_flow_amd import frame_pairs, synthetic, utils_eval
    tmp = tmp_path_factory.mktemp("segments")
    d = synthetic.make_sequence(seed=3, num_frames=3, n_objects=6, n_max=400)
    sd = (d["nonground"] & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    os.makedirs(os.path.join(tmp, "val"))
    path = os.path.join(tmp, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=d["nonground"].astype(np.int64))
    a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.05, False, "ego_motion_gt"
    plain = frame_pairs.run_sequences(a, [path], DEV)
    v = SimpleNamespace(**vars(a))
    v.if_verbose = True
    tables = []
    real = utils_eval.sequence_table

    def spy(args, data, flow_seq):
        out = real(args, data, flow_seq)
        if int(args.num_frames) == 3:
            tables.append(out)
        return out

    utils_eval.sequence_table = spy
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            verbose = frame_pairs.run_sequences(v, [path], DEV)
    finally:
        utils_eval.sequence_table = real
    return dict(path=path, dir=str(tmp), args=a, plain=plain, verbose=verbose, table=tables[0], text=text.getvalue())


def test_segments_sum_to_the_sequence_table(sequence_runs):
    """Per gap j: the segments' kept rows and each predicate count sum to icpflow_seq_metrics' row j, class overall, exactly; the
    sums of e agree within (n - 1) 2^-53 sum e on each side; every meter equals the run without the flag, field by field."""
    from icp_flow_amd import utils_eval
    r = sequence_runs
    assert "segments" not in r["plain"] and "ms_report_per_sequence" not in r["plain"]
    reports = r["verbose"]["segments"]
    assert [x["gap"] for x in reports] == [1, 2] and r["verbose"]["ms_report_per_sequence"] > 0
    table, esum = r["table"][0], r["table"][1]
    for rep in reports:
        j, seg = rep["gap"], rep["segments"]
        n = int(table[j, 0, 0])
        assert n > 0 and int(seg.n.sum()) == n
        with np.errstate(all="ignore"):
            counts = [np.nan_to_num(np.round(getattr(seg, k).astype(np.float64) * seg.n)).sum() for k in ("accs", "accr", "outlier", "routlier")]
        assert [int(c) for c in counts] == [int(table[j, 0, 2 + k]) for k in range(4)]
        total = math.fsum(seg.sum_e)
        print(f"gap {j}: {len(seg)} segments, kept {n}, sum e {total!r} vs {esum[j, 0]!r}")
        assert abs(total - esum[j, 0]) <= (n - 1) * sg.U * esum[j, 0]
        assert rep["frame"]["overall"][5] == n and {-1e8} <= set(seg.label.tolist())
        assert any(line.startswith("eval segment:") for line in seg.lines)
    assert "debug frame: 1/3,  overall, EPE: " in r["text"] and "eval segment:" in r["text"]
    for name, got in r["verbose"]["metrics"].items():
        ref = r["plain"]["metrics"][name]
        assert got.num == ref.num and got.num_data == ref.num_data, name
        for m in utils_eval.METRIC_NAMES:
            for field in ("_sum", "_avg", "_data"):
                a, b = np.asarray(getattr(got, m + field), np.float64), np.asarray(getattr(ref, m + field), np.float64)
                assert np.array_equal(a, b, equal_nan=True), (name, m, field)


def test_report_lists_exactly_the_segments_above_the_threshold(sequence_runs, monkeypatch, capsys):
    """--report through the command line: the file holds exactly the segments above --report-epe, worst first."""
    from icp_flow_amd import frame_pairs
    r = sequence_runs
    reports = r["verbose"]["segments"]
    every = sorted(float(e) for rep in reports for e in rep["segments"].epe if not np.isnan(e))
    threshold = every[len(every) // 2] if len(every) > 1 else 0.0      # about half of the segments above it
    want = [(rep["gap"], float(rep["segments"].label[k])) for rep in reports for k in range(len(rep["segments"]))
            if rep["segments"].epe[k] > threshold]
    assert 0 < len(want) < len(every)
    listed = frame_pairs.worst_segments(reports, threshold)
    assert sorted((x["gap"], x["label"]) for x in listed) == sorted(want)
    assert [x["epe"] for x in listed] == sorted((x["epe"] for x in listed), reverse=True)
    out = os.path.join(r["dir"], "worst.json")
    a = r["args"]
    frame_pairs.main([r["dir"], "--protocol", "reference", "--cluster", "dbscan", "--max-points", "1024", "--speed", "1.67", "--min-cluster-size", "20",
                      "--range-x", "80", "--range-y", "80", "--epsilon", "0.8", "--num-frames", "3", "--ground-slack", "0.05", "--pose-source",
                      "ego_motion_gt", "--if-verbose", "--report", out, "--report-epe", repr(threshold)])
    text = capsys.readouterr().out
    assert "debug frame: 1/3,  overall" in text and "eval segment:" in text and "overall_0" in text and a.num_frames == 3
    with open(out) as f:
        rows = json.load(f)
    assert [(x["gap"], x["label"], x["n"], x["epe"]) for x in rows] == [(x["gap"], x["label"], x["n"], x["epe"]) for x in listed]
    assert all(set(x) >= {"sequence", "gap", "label", "n", "epe", "matched_label", "translation", "rotation_zyx_deg"} for x in rows)

"""CPU-only part of the Argoverse 2 path (icpflow_seq_argo_sample, utils_loading.argo_sample, frame_pairs.load_argo_sample,
run_sequences(dataset="argo"), --dataset argo): the ABI, argument errors, the refusal without a GPU, the numpy restatement
(tests/argo_restatement.py) against the g15 fixtures = the reference's own dataset_argo / calculate_metrics
(tools/gen_golden_argo.py), the association order of numpy's norm, the fixtures' margin conditions, and the command line."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import argo_restatement as ar         # noqa: E402
import seqeval_restatement as sr      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = list(ar.SYNTHETIC) + [ar.DEMO]


def test_the_symbol_is_declared_bound_and_exported():
    import __graft_entry__ as entry
    from icp_flow_amd import _lib
    lib = ctypes.CDLL(entry.build())
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "icpflow_hip.h")).read(), flags=re.S)
    name = "icpflow_seq_argo_sample"
    assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared"
    assert hasattr(lib, name), f"{name} not exported"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 22, f"{name} not bound"
    assert _lib.VERSION == 215 and "#define ICPFLOW_VERSION 215" in hdr
    assert "#define ICPFLOW_ARGO_MAX_BACKGROUND 64" in hdr and _lib.ARGO_MAX_BACKGROUND == 64
    assert "#define ICPFLOW_DTYPE_FLOAT32 0" in hdr and "#define ICPFLOW_DTYPE_FLOAT64 1" in hdr
    assert (_lib.DTYPE_FLOAT32, _lib.DTYPE_FLOAT64) == (0, 1)


def test_refusals_are_status_codes_with_messages():
    """Every refusal happens before any launch: the pointers here point nowhere."""
    from icp_flow_amd import _lib
    L, one = _lib._L, ctypes.c_void_p(64)
    bg = (ctypes.c_int32 * 65)(*range(65))

    def call(n1=10, n2=10, pd=0, fd=0, m1=4, m2=4, nbg=6, pc1=one, pc2=one, flow=one, cls=one, v1=one, v2=one, hbg=bg, out=one, bad=one):
        return L.icpflow_seq_argo_sample(pc1, n1, pc2, n2, pd, flow, fd, cls, v1, m1, v2, m2, hbg, nbg, 0.05, out, out, out, out, out, bad, None)

    for kw in (dict(n1=-1), dict(n2=-1), dict(m1=-1), dict(m2=-1)):
        assert call(**kw) == -1 and b"must be >= 0" in L.icpflow_last_error(), kw
    assert call(nbg=-1) == -1 and b"n_background < 0" in L.icpflow_last_error()
    for kw in (dict(pd=2), dict(fd=-1), dict(pd=7, fd=7)):
        assert call(**kw) == -1 and b"dtype" in L.icpflow_last_error(), kw
    assert call(nbg=65) == -3 and b"65 background classes" in L.icpflow_last_error()
    for kw in (dict(bad=None), dict(pc1=None), dict(flow=None), dict(cls=None), dict(v1=None), dict(pc2=None), dict(v2=None),
               dict(out=None), dict(hbg=None), dict(m1=0, m2=0, bad=None)):
        assert call(**kw) == -1 and b"icpflow_seq_argo_sample: null pointer" in L.icpflow_last_error(), kw


def _write_file(tmp_path, name):
    arrays, _ = ar.file_arrays(name)
    path = os.path.join(tmp_path, name + ".npz")
    np.savez(path, **arrays)
    return path


def test_without_a_gpu_the_sample_is_refused(tmp_path, monkeypatch):
    from icp_flow_amd import frame_pairs, utils_loading
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    path = _write_file(tmp_path, "g15_argo_f32_int")
    assert frame_pairs.is_argo(path)
    for device in ("cuda:0", "cpu", None):
        with pytest.raises(RuntimeError, match="no CPU path"):
            frame_pairs.load_argo_sample(path, frame_pairs.default_args(), device)
    arrays, _ = ar.file_arrays("g15_argo_f32_int")
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_loading.argo_sample(T(arrays["pc1"]), T(arrays["pc2"]), T(arrays["gt_flow_0_1"]), T(arrays["pc1_classes"]),
                                  T(arrays["pc1_flows_valid_idx"]), T(arrays["pc2_flows_valid_idx"]))


def _restated(name):
    arrays, pred = ar.file_arrays(name)
    g = ar.load(name)
    got = ar.sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"], arrays["pc1_flows_valid_idx"],
                    arrays["pc2_flows_valid_idx"], g["background_idxes"])
    return arrays, pred, got


@pytest.mark.parametrize("name", FIXTURES)
def test_the_restatement_equals_the_reference(name):
    """What dataset_argo.load_data_pca returned for the file, key by key"""
    _, _, got = _restated(name)
    want = ar.recorded_sample(name)
    for k in ar.SAMPLE_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    rows = got["time_indice"] == 1
    sd, fb = got["sd_labels"][rows] == 1, got["fb_labels"][rows] == 1
    assert all(x.any() for x in (sd & fb, ~sd & fb, ~sd & ~fb))          # dynamic, static, fg and bg all have members
    if name == ar.DEMO:      # what the issue states about the real sample
        assert (int(sd.sum()), int((sd & fb).sum()), int((~sd & fb).sum())) == (4250, 4250, 414)
    else:
        assert (sd & ~fb).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_norms_association_order_is_numpys(dtype):
    """Rows whose (x x + y y) + z z and x x + (y y + z z) round differently and fall on different sides of 0.05 in their
    dtype: the restatement's labels are np.linalg.norm's -- numpy adds from the left."""
    rows = ar.straddling_rows(dtype)
    assert rows.dtype == dtype and len(rows) >= 1000
    want = np.linalg.norm(rows, axis=-1) > (0.5 * 0.1)
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    other = np.sqrt(x * x + (y * y + z * z)) > ar.sd_threshold(dtype)
    assert (want != other).all() and 0.3 < want.mean() < 0.7
    n = len(rows)
    got = ar.sample(rows, rows[:0], rows, np.zeros(n), np.arange(n), np.arange(0), ())
    assert np.array_equal(got["sd_labels"], want.astype(np.int32)) and (got["fb_labels"] == 1).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_margin_conditions(name):
    """tools/gen_golden_argo.py's MARGIN CONDITIONS from the stored values: no |flow| within 1e-6 (relative) of 0.05, no e or
    r within 1e-9 (relative) of a predicate threshold -- a last-bit difference cannot move a point across."""
    want = ar.recorded_sample(name)
    _, pred = ar.file_arrays(name)
    rows = want["time_indice"] == 1
    gt = want["scene_flow"][rows]
    norm = np.linalg.norm(gt, axis=-1)
    assert (np.abs(norm - 0.05) > 1e-6 * 0.05).all() and 0 < (norm > 0.05).sum() < len(norm)
    e, r = sr.errors(gt, pred[rows])
    for thr in (0.05, 0.1, 0.3):
        assert (np.abs(e - thr) > 1e-9 * thr).all() and (np.abs(r - thr) > 1e-9 * thr).all()
        assert 0 < (e < thr).sum() < len(e)
    assert want["scene_flow"].dtype == np.float64 and pred.dtype == np.float32 and (pred[~rows] == 0).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_the_default_background_list_is_the_recorded_one(name):
    from icp_flow_amd import utils_loading
    assert list(utils_loading.ARGO_BACKGROUND_IDXES) == ar.load(name)["background_idxes"].tolist()
    assert float(ar.sd_threshold(np.float64)) == utils_loading.ARGO_DYNAMIC_THRESHOLD


@pytest.mark.parametrize("setting", list(ar.SETTINGS))
@pytest.mark.parametrize("name", FIXTURES)
def test_meters_of_the_restated_sample_equal_the_reference(name, setting):
    """The restated sample (points in the file's dtype, as the product hands them on) -> the numpy statement of the table
    (tests/seqeval_restatement.py) -> the existing host half (table -> meters): every meter as the reference's
    calculate_metrics left it on load_data_pca's sample."""
    from icp_flow_amd import utils_eval
    arrays, pred, got = _restated(name)
    data = dict(got, raw_points=got["raw_points"].astype(arrays["pc1"].dtype))
    args = ar.setting_args(setting)
    table, esum, kept0 = sr.table_numpy(args, data, pred)
    rec = ar.Recorded(ar.load(name), setting)
    want, _, want_kept0 = sr.reference_table(rec, 0)
    assert np.array_equal(table, want) and kept0 == want_kept0
    assert table[0, 4, 0] > 0 and table[0, 3, 0] > 0 and table[0, 2, 0] > 0
    meters = utils_eval.update_meters(args, utils_eval.new_metric_table(2), table, esum, kept0)
    sr.check_meters(meters, rec, 0, lambda v, n: 2 * n * sr.U * v)
    assert len(utils_eval.format_metric_table(meters, 2).split("\n")) == 1 + 18


def test_command_line_selects_files_by_dataset(tmp_path, monkeypatch):
    """--protocol reference without --dataset hands run_sequences what it did before for a directory mixing both kinds (the
    sequence files); --dataset argo the Argoverse files with num_frames 2; another --num-frames exits."""
    from icp_flow_amd import frame_pairs, synthetic, utils_eval
    seq = os.path.join(tmp_path, "a_seq.npz")
    np.savez(seq, **synthetic.make_sequence(seed=5, num_frames=3, n_objects=2, n_max=60, n_background=50))
    argo = _write_file(tmp_path, "g15_argo_f32_float")
    d = synthetic.make_frame_pair(seed=1, n_objects=2, n_max=60, n_background=50)
    np.savez(os.path.join(tmp_path, "pair.npz"), **{k: d[k] for k in ("points_src", "points_dst", "labels_src", "labels_dst")})
    assert [frame_pairs.is_argo(p) for p in frame_pairs.list_frame_pairs(str(tmp_path))] == [False, True, False]
    assert not frame_pairs.is_sequence(argo)
    calls = []

    def fake(args, paths, device, in_flight=1, **kw):
        calls.append((list(paths), kw, args.num_frames, (args.range_x, args.range_y, args.range_z, args.ground_slack, args.eval_ground)))
        return dict(metrics=utils_eval.new_metric_table(args.num_frames), sequences=len(paths))

    monkeypatch.setattr(frame_pairs, "run_sequences", fake)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    frame_pairs.main([str(tmp_path), "--protocol", "reference"])
    assert calls[-1] == ([seq], {}, 5, (32.0, 32.0, 0.0, 0.3, False))
    frame_pairs.main([str(tmp_path), "--protocol", "reference", "--dataset", "pca", "--num-frames", "3"])
    assert calls[-1] == ([seq], {}, 3, (32.0, 32.0, 0.0, 0.3, False))
    frame_pairs.main([str(tmp_path), "--protocol", "reference", "--dataset", "argo"])
    assert calls[-1] == ([argo], dict(dataset="argo"), 2, (32.0, 32.0, 0.0, 0.3, False))
    frame_pairs.main([str(tmp_path), "--protocol", "reference", "--dataset", "argo", "--num-frames", "2", "--range-x", "10000",
                      "--range-y", "10000", "--range-z", "-10000", "--ground-slack", "0"])
    assert calls[-1] == ([argo], dict(dataset="argo"), 2, (10000.0, 10000.0, -10000.0, 0.0, False))
    n = len(calls)
    for argv in (["--protocol", "reference", "--dataset", "argo", "--num-frames", "5"], ["--dataset", "argo", "--num-frames", "5"],
                 ["--dataset", "argo"]):
        with pytest.raises(SystemExit):
            frame_pairs.main([str(tmp_path)] + argv)
    assert len(calls) == n


def test_run_sequences_refuses_another_frame_count():
    from icp_flow_amd import frame_pairs
    a = frame_pairs.default_args()
    a.num_frames = 5
    with pytest.raises(ValueError, match="two frames"):
        frame_pairs.run_sequences(a, [], "cuda:0", dataset="argo")
    with pytest.raises(ValueError, match="dataset"):
        frame_pairs.run_sequences(a, [], "cuda:0", dataset="waymo")

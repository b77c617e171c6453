"""The per-segment evaluation without a GPU: the ABI of icpflow_seq_segment_table (symbols, status codes before any launch,
workspace sizes), the numpy restatement and the host half of utils_flow.flow_evaluation against the g14 fixtures -- the
reference's own flow_evaluation / debug_frame run on the CPU by tools/gen_golden_segments.py."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_restatement as sg      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("icpflow_seq_segment_table_workspace_bytes", "icpflow_seq_segment_table")


def test_symbols_exported_declared_and_bound():
    from icp_flow_amd import _lib, build
    hdr = open(os.path.join(REPO, "include", "icpflow_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES, f"{name} not bound"
    assert "#define ICPFLOW_SEG_COLS 16" in hdr and _lib.SEG_COLS == 16 == sg.COLS
    assert _lib.SEG_CHUNK_ROWS == sg.CHUNK and "constexpr int kChunk = %d;" % sg.CHUNK in open(os.path.join(build.CSRC, "segeval.hip")).read()
    assert "segeval.hip" in build.SOURCES and "rowerr.hpp" in build.HEADERS
    assert _lib.VERSION == 215
    # the per-row arithmetic is one function that both kernels call
    for src in ("seqeval.hip", "segeval.hip"):
        text = open(os.path.join(build.CSRC, src)).read()
        assert '#include "rowerr.hpp"' in text and "icpflow::row_error(" in text


def _call(n=10, Lmax=64, pts=1, lab=1, gt=1, pd=1, table=1, num=1, ws=1, nbytes=None):
    """the entry point on made-up non-null host addresses: every refusal below comes before a launch, no device is touched"""
    from icp_flow_amd import _lib
    L = _lib._L
    a = lambda on: ctypes.c_void_p(0x1000 if on else 0)   # noqa: E731
    if nbytes is None:
        nbytes = L.icpflow_seq_segment_table_workspace_bytes(max(n, 0), min(max(Lmax, 1), 4096))
    rc = L.icpflow_seq_segment_table(a(pts), a(lab), n, a(gt), a(pd), 0.3, a(table), Lmax, a(num), a(ws), ctypes.c_size_t(nbytes), None)
    return rc, L.icpflow_last_error()


def test_status_codes_before_any_launch():
    from icp_flow_amd import _lib
    rc, msg = _call(n=-1)
    assert rc == -1 and b"n < 0" in msg
    for Lmax in (0, -3, 4097):
        rc, msg = _call(Lmax=Lmax)
        assert rc == -3 and b"Lmax" in msg and str(Lmax).encode() in msg
    for kw in (dict(table=0), dict(num=0), dict(pts=0), dict(lab=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and b"null pointer" in msg, kw
    for kw in (dict(gt=0), dict(pd=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and b"together" in msg, kw
    need = _lib._L.icpflow_seq_segment_table_workspace_bytes(5000, 64)
    rc, msg = _call(n=5000, nbytes=need - 1)
    assert rc == -2 and b"workspace" in msg and str(need).encode() in msg
    rc, msg = _call(ws=0)
    assert rc == -2 and b"workspace" in msg


def _expected_workspace(n, Lmax):
    """the carve of csrc/segeval.hip: order, (label, count, start) rows, chunk starts, partials of 12 doubles per chunk, then
    table.hip's own (two arrays of Lmax words, a uint16 per row, Lmax counts per chunk of 512 rows), regions of 256-byte multiples"""
    al = lambda b: -(-b // 256) * 256   # noqa: E731
    chunks = n // sg.CHUNK + min(n, Lmax) + 1
    own = al(n * 8) + al(Lmax * 9 * 8) + al((Lmax + 1) * 4) + al(chunks * 12 * 8)
    sort = 4 * al(Lmax * 4) + al(n * 2) + al(-(-n // 512) * Lmax * 4)
    return own + al(sort)


# recorded from the library as built from this tree
PINNED_SIZES = {(0, 1): 1792, (1, 1): 2560, (1000, 64): 23296, (1024, 64): 23296, (1025, 64): 24064, (5000, 64): 65792,
                (5000, 4096): 985088, (65536, 1024): 1378816, (200000, 4096): 9195520}


def test_workspace_sizes_aligned_monotone_and_pinned():
    from icp_flow_amd import _lib
    ws = _lib._L.icpflow_seq_segment_table_workspace_bytes
    assert ws(-1, 8) == 0 and ws(10, 0) == 0 and ws(10, 4097) == 0
    for (n, Lmax), want in PINNED_SIZES.items():
        got = ws(n, Lmax)
        print(f"({n}, {Lmax}): {got}")
        assert got == _expected_workspace(n, Lmax), (n, Lmax, got, _expected_workspace(n, Lmax))
        assert got == want and got % 256 == 0, (n, Lmax, got)
    for Lmax in (1, 64, 4096):
        sizes = [ws(n, Lmax) for n in (0, 1, 63, 1023, 1024, 1025, 5000, 65536, 200000)]
        assert sizes == sorted(sizes)
    for n in (0, 1, 5000, 200000):
        sizes = [ws(n, Lmax) for Lmax in (1, 2, 64, 1024, 4096)]
        assert sizes == sorted(sizes)


@pytest.mark.parametrize("name", sg.FIXTURES)
def test_margin_condition_on_the_stored_values(name):
    g = sg.load(name)
    assert sg.margin(g)
    assert g["flow_gt"].dtype == np.float64 and g["flow_pd"].dtype == np.float32
    assert g["src_points"].dtype == (np.float32 if name.endswith("f32") else np.float64)
    assert np.nanmax(g["crop_epe"]) > 2.0                      # the "substantially large flow errors" block is exercised
    assert 23 in g["all_labels"] and 23 not in g["crop_labels"]   # a cluster entirely below z_min
    assert {-100000000, -1} <= set(g["crop_labels"].tolist())
    matched = set(g["pairs"][:, 0].astype(int).tolist())
    clusters = set(g["crop_labels"][g["crop_labels"] >= 0].tolist())
    assert clusters & matched and clusters - matched           # some matched, some not


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "all"])
@pytest.mark.parametrize("name", sg.FIXTURES)
def test_restatement_reproduces_g14(name, crop):
    """Counts and the float32 fractions exactly; EPE and the means within the bound of two summation orders in the precision the
    reference adds in (normally equal: the same numpy expressions)."""
    g = sg.load(name)
    tag = "crop_" if crop else "all_"
    got = sg.reference_numbers(g, crop)
    assert np.array_equal(got["labels"], g[tag + "labels"])
    assert np.array_equal(got["len_i"], g[tag + "len_i"]) and np.array_equal(got["len_j"], g[tag + "len_j"])
    for k in ("accs", "accr", "outlier", "routlier"):
        assert all(sg.same_f32(a, b) for a, b in zip(got[k], g[tag + k])), k
    n = g[tag + "len_i"]
    assert (np.abs(got["epe"] - g[tag + "epe"]) <= sg.mean_bound(n, g[tag + "epe"], np.float64)).all()
    dt = g["src_points"].dtype
    for k, cnt in (("mean_i", n), ("mean_j", g[tag + "len_j"]), ("moved", n)):
        a, b = got[k], g[tag + k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = np.abs(a - b) <= sg.mean_bound(cnt[:, None], 45.0, dt)       # (|coordinate| + |flow| stay below 45 m in the fixture)
        assert (ok | np.isnan(a)).all(), k
    assert (np.abs(got["translation"] - g[tag + "translation"]) <= 6 * sg.mean_bound(n, 45.0, dt)).all()
    fr, want = got["frame_rows"], g[tag + "frame_rows"]
    assert np.array_equal(fr[:, 5], want[:, 5])
    assert all(sg.same_f32(a, b) for a, b in zip(fr[:, 1:5].ravel(), want[:, 1:5].ravel()))
    assert (np.abs(fr[:, 0] - want[:, 0]) <= sg.mean_bound(want[:, 5], want[:, 0], np.float64)).all()
    # the table the kernel is checked against says the same: counts of the kept rows, fractions from its counts
    table, e, _, _ = sg.table_numpy(g["src_points"], g["src_labels"], g["flow_pd"], g["flow_gt"], float(g["z_min"]) if crop else None)
    kept = table[table[:, 2] > 0]
    assert np.array_equal(kept[:, 0].astype(np.int64), g[tag + "labels"]) and np.array_equal(kept[:, 2].astype(np.int64), n)
    for k, col in (("accs", 4), ("accr", 5), ("outlier", 6), ("routlier", 7)):
        frac = kept[:, col].astype(np.float32) / kept[:, 2].astype(np.float32)
        assert all(sg.same_f32(a, b) for a, b in zip(frac, g[tag + k])), k


@pytest.mark.parametrize("name", sg.FIXTURES)
def test_euler_angles_in_closed_form(name):
    from icp_flow_amd import utils_flow
    g = sg.load(name)
    for T, want in zip(g["transformations"], g["euler_zyx_deg"]):
        assert np.abs(utils_flow.euler_zyx_deg(T[0:3, 0:3]) - want).max() <= 1e-9
    assert np.abs(g["euler_zyx_deg"]).max() > 1.0
    assert np.abs(utils_flow.euler_zyx_deg(np.eye(3))).max() == 0.0


def _report(g, crop):
    """the host half of flow_evaluation on the restatement's tables"""
    from icp_flow_amd import utils_flow
    src, _, _, _ = sg.table_numpy(g["src_points"], g["src_labels"], g["flow_pd"], g["flow_gt"], float(g["z_min"]) if crop else None)
    dst, _, _, _ = sg.table_numpy(g["dst_points"], g["dst_labels"])
    rep = utils_flow.segment_report(src, dst, g["pairs"], g["transformations"])
    rep.lines = utils_flow.segment_lines(rep, rep.moved, g["pose"], g["transformations"], g["pairs"])
    return rep


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "all"])
@pytest.mark.parametrize("name", sg.FIXTURES)
def test_host_half_of_the_report_and_its_lines(name, crop):
    g = sg.load(name)
    rep = _report(g, crop)
    sg.check_report(rep, g, crop)
    sg.check_lines(rep.lines, g, crop)
    worst = rep.worst(2.0)
    assert [w["label"] for w in worst] == [57.0] and worst[0]["matched_label"] == 57.0 and worst[0]["epe"] > 2.0
    assert rep.worst(0.0)[0]["label"] == 57.0 and len(rep.worst(0.0)) == int((rep.n > 0).sum())


@pytest.mark.parametrize("name", sg.FIXTURES)
def test_frame_lines_as_the_reference_prints_them(name):
    from icp_flow_amd import utils_debug
    g = sg.load(name)
    for crop, tag in ((True, "crop_"), (False, "all_")):
        rows = {k: (np.float64(v[0]),) + tuple(np.float32(x) for x in v[1:5]) + (int(v[5]),)
                for k, v in zip(utils_debug.FRAME_CLASSES, g[tag + "frame_rows"])}
        lines = utils_debug.frame_lines(SimpleNamespace(num_frames=2), 1, rows)
        assert lines == str(g[tag + "frame_text"]).strip().split("\n")


def test_run_sequences_without_the_flag_and_cpu_tensors(tmp_path, monkeypatch):
    """Without if_verbose run_sequences returns no `segments` key and calls nothing of the report; CPU tensors are refused."""
    from icp_flow_amd import frame_pairs, synthetic, utils_debug, utils_flow
    g = sg.load("g14_segments_f64")
    T = torch.from_numpy
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_flow.segment_table(T(g["src_points"]), T(g["src_labels"]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_flow.flow_evaluation(T(g["src_points"]), T(g["dst_points"]), T(g["src_labels"]), T(g["dst_labels"]), T(g["flow_pd"]),
                                   T(g["flow_gt"]), T(g["pose"]), T(g["transformations"]), pairs=T(g["pairs"]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_debug.frame_rows(SimpleNamespace(eval_ground=True), T(g["src_points"]), T(g["sd_label"]), T(g["fb_label"]), T(g["flow_gt"]),
                               T(g["flow_pd"]))
    d = synthetic.make_sequence(seed=5, num_frames=3, n_objects=4, n_max=120, n_background=150)
    os.makedirs(os.path.join(tmp_path, "val"))
    path = os.path.join(tmp_path, "val", "s0.npz")
    np.savez(path, **d, sd_labels=np.zeros(len(d["raw_points"]), np.int64), fb_labels=np.zeros(len(d["raw_points"]), np.int64))
    a = frame_pairs.default_args(speed=0.8333, range_x=30.0, range_y=30.0)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.3, False, "ego_motion_gt"
    called = []

    def register(args, fp, device, gap=None):
        return dict(pairs=torch.zeros((0, 10)), transformations=torch.zeros((0, 4, 4)), flow=torch.from_numpy(fp.gt_flow))

    monkeypatch.setattr(frame_pairs, "register_frame_pair", register)
    monkeypatch.setattr(frame_pairs.utils_eval, "calculate_metrics", lambda *a, **k: called.append("metrics"))
    monkeypatch.setattr(frame_pairs, "_sequence_reports", lambda *a, **k: called.append("report") or [])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    res = frame_pairs.run_sequences(a, [path], "cpu")
    assert "segments" not in res and "ms_report_per_sequence" not in res and called == ["metrics"]
    assert sorted(res) == ["frame_pairs", "ground", "metrics", "ms_eval_per_sequence", "ms_per_sequence", "pose_sources", "sequences"]
    a.if_verbose = True
    called.clear()
    res = frame_pairs.run_sequences(a, [path], "cpu")
    assert called == ["metrics", "report"] and res["segments"] == [] and res["ms_report_per_sequence"] >= 0

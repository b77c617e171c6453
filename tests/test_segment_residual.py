"""CPU-only: the nearest-neighbour residual per segment (icpflow_nn_residual_segments, csrc/segresid.hip;
utils_eval.segment_residual; run_stream's `--residual-segments`) as far as it goes without a GPU -- the exports, every argument
refusal with its code and message (all of them come before any launch), the pinned size query against the header's formula,
the command line, SegmentResidual.worst on a hand-made table, the restatement the GPU tests compare against
(tests/segment_residual_restatement.py) on a scene counted by hand, and the conditions the GPU tests' scenes must meet
(tests/segment_residual_cases.py), asserted on the restatement."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_restatement as rr             # noqa: E402
import segment_residual_cases as cases        # noqa: E402
import segment_residual_restatement as sr     # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "workspace_sizes_nn_residual_segments.json")
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
FN = "icpflow_nn_residual_segments"


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib, build
    assert _lib.VERSION == 215
    for name, n_args in ((FN + "_workspace_bytes", 4), (FN, 19)):
        assert hasattr(_lib._L, name) and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES[FN + "_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.NNRS_COLS, _lib.NNRS_MAX_SEGMENTS) == (18, 4096)
    assert "segresid.hip" in build.SOURCES and "nnresid.hpp" in build.HEADERS
    hdr = open(os.path.join(REPO, "include", "icpflow_hip.h")).read()
    assert "#define ICPFLOW_NNRS_COLS 18" in hdr


def _call(**over):
    """the call with arguments that pass every check but the workspace's size (16 bytes: nothing is launched), `over`
    replacing some.  -> (status, message)"""
    from icp_flow_amd import _lib
    one = ctypes.c_void_p(4096)
    edges = np.asarray(over.pop("edges", (0.05, 0.1)), np.float64)
    a = dict(before=one, after=one, flow=None, labels=one, n=10, target=one, m=10, radius=2.0,
             h_edges=edges.ctypes.data_as(ctypes.c_void_p) if len(edges) else None, E=len(edges), table=one, Lmax=64, num=one, d2b=one, d2a=one,
             info=one, ws=one, ws_bytes=16)
    a.update(over)
    rc = getattr(_lib._L, FN)(a["before"], a["after"], a["flow"], a["labels"], a["n"], a["target"], a["m"], a["radius"], a["h_edges"], a["E"],
                              a["table"], a["Lmax"], a["num"], a["d2b"], a["d2a"], a["info"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    return rc, _lib._L.icpflow_last_error().decode()


def test_every_refusal_has_its_code_and_message():
    from icp_flow_amd import _lib
    # what passes every argument check stops at the workspace: the refusals below are not that one
    rc, msg = _call()
    assert rc == E_WORKSPACE and FN + "_workspace_bytes" in msg
    rc, msg = _call(ws=None, ws_bytes=1 << 30)
    assert rc == E_WORKSPACE and "workspace" in msg
    for over in (dict(before=None), dict(after=None), dict(labels=None), dict(target=None), dict(info=None), dict(table=None), dict(num=None),
                 dict(h_edges=None)):
        rc, msg = _call(**over)
        assert rc == E_ARG and FN + ": null pointer" in msg, over
    # a cloud without rows needs no pointer; the optional arguments may be NULL, each and together
    assert _call(before=None, after=None, labels=None, n=0)[0] == E_WORKSPACE and _call(target=None, m=0)[0] == E_WORKSPACE
    for over in (dict(d2b=None), dict(d2a=None), dict(d2b=None, d2a=None), dict(flow=ctypes.c_void_p(4096))):
        assert _call(**over)[0] == E_WORKSPACE, over
    for over in (dict(n=-1), dict(m=-1)):
        rc, msg = _call(**over)
        assert rc == E_ARG and "< 0" in msg, over
    for r in (0.0, 0.99e-3, 1000.5, -2.0, float("nan"), float("inf")):
        rc, msg = _call(radius=r)
        assert rc == E_ARG and "radius" in msg and "[1e-3, 1e3]" in msg, r
    assert _call(radius=1e-3, edges=())[0] == E_WORKSPACE and _call(radius=1e3)[0] == E_WORKSPACE
    for Lmax in (0, -1):
        rc, msg = _call(Lmax=Lmax)
        assert rc == E_ARG and "Lmax must be at least 1" in msg, Lmax
    for Lmax in (4097, 1 << 20):
        rc, msg = _call(Lmax=Lmax)
        assert rc == E_LIMIT and "at most 4096 segments" in msg, Lmax
    assert _call(Lmax=1)[0] == E_WORKSPACE and _call(Lmax=4096)[0] == E_WORKSPACE
    rc, msg = _call(edges=(0.01, 0.02, 0.03, 0.04, 0.05))
    assert rc == E_ARG and "E must lie in [0, 4]" in msg
    rc, msg = _call(E=-1)
    assert rc == E_ARG and "E must lie in [0, 4]" in msg
    assert _call(edges=(0.01, 0.02, 0.03, 2.0))[0] == E_WORKSPACE and _call(edges=())[0] == E_WORKSPACE
    for edges in ((0.1, 0.05), (0.05, 0.05), (float("nan"), 0.1), (0.05, float("inf")), (0.05, 2.5), (0.0, 0.1), (-0.1, 0.1)):
        rc, msg = _call(edges=edges)
        assert rc == E_ARG and "edges must be finite, positive, strictly ascending and at most the radius" in msg, edges
    for over in (dict(m=(1 << 29) + 1), dict(n=(1 << 29) + 1)):
        rc, msg = _call(**over)
        assert rc == E_LIMIT and "rows a cloud" in msg, over
    need = getattr(_lib._L, FN + "_workspace_bytes")(10, 10, 64, 2)
    rc, msg = _call(ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    assert rc == E_ARG and "16-byte aligned" in msg
    assert all(FN in _call(**over)[1] for over in (dict(n=-1), dict(radius=0.0), dict(Lmax=0), dict(E=9), dict(edges=(0.2, 0.1))))


def _formula(n, m, Lmax, E):
    """the size as include/icpflow_hip.h states it"""
    from icp_flow_amd import _lib
    a = lambda x: -(-x // 256) * 256   # noqa: E731

    def table(k):
        H = 1
        while H < 2 * k:
            H *= 2
        return 2 * a(4 * H) + 4 * a(4 * -(-H // 1024)) + 256 + a(16 * k)

    chunks = n // 1024 + min(n, Lmax) + 1
    T = _lib._L.icpflow_cluster_table_workspace_bytes(max(n, 1), Lmax)
    return table(m) + table(n) + 3 * a(4 * n) + a(8 * n) + a(72 * Lmax) + a(4 * (Lmax + 1)) + a(128 * chunks) + a(T)


def test_the_size_query_is_pinned_and_monotone():
    from icp_flow_amd import _lib
    q = getattr(_lib._L, FN + "_workspace_bytes")
    recorded = json.load(open(GOLDEN))[FN + "_workspace_bytes"]
    assert len(recorded) >= 100
    for n, m, Lmax, E, size in recorded:
        assert q(n, m, Lmax, E) == size == _formula(n, m, Lmax, E) and size % 256 == 0 and size > 0, (n, m, Lmax, E)
    sizes = [0, 1, 63, 64, 65, 511, 512, 513, 2049, 20000, 63276, 130000, 1 << 20]
    for Lmax, E in ((1, 0), (64, 2), (4096, 4)):
        for m in sizes:
            by_n = [q(n, m, Lmax, E) for n in sizes]
            assert by_n == sorted(by_n), (m, Lmax, E)
        for n in sizes:
            by_m = [q(n, m, Lmax, E) for m in sizes]
            assert by_m == sorted(by_m), (n, Lmax, E)
            assert len({q(n, 100, Lmax, e) for e in range(5)}) == 1           # E does not enter
    # arguments the call refuses
    assert q(-1, 1, 1, 0) == 0 and q(1, -1, 1, 0) == 0 and q(1, 1, 0, 0) == 0 and q(1, 1, 4097, 0) == 0 and q(1, 1, 1, 5) == 0 and q(1, 1, 1, -1) == 0
    assert q(1, (1 << 29) + 1, 1, 0) == 0 and q((1 << 29) + 1, 1, 1, 0) == 0


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_eval
    x, lab = torch.zeros(8, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.segment_residual(x, x, x, lab, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.segment_residual_device(x, x, None, lab, x)


def test_the_flag_parses_bare_and_with_a_file():
    from icp_flow_amd import frame_pairs
    ap = frame_pairs.argument_parser()
    assert ap.parse_args(["dir"]).residual_segments is None
    assert ap.parse_args(["dir", "--residual", "--residual-segments"]).residual_segments is True
    ns = ap.parse_args(["dir", "--residual", "0.5", "--residual-segments", "worst.json"])
    assert ns.residual_segments == "worst.json" and ns.residual == 0.5
    with pytest.raises(SystemExit, match="--residual-segments goes with --residual"):
        frame_pairs.main(["dir", "--residual-segments"])
    with pytest.raises(SystemExit, match="--residual-segments goes with --residual"):
        frame_pairs.main(["dir", "--residual-segments", "worst.json"])
    assert "residual_segments" not in frame_pairs.DEFAULT_ARGS and not hasattr(frame_pairs.default_args(), "residual_segments")


def test_a_scene_counted_by_hand():
    """three segments, two edges, radius 1, targets on the x axis; every number below is worked out by hand (dyadic: exact)"""
    target = np.array([[0, 0, 0], [1, 0, 0], [10, 0, 0], [1e8, 1e8, 1e8]], np.float32)
    before = np.array([[0.25, 0, 0],      # label 5: d 0.25 from target 0;          the flow takes it onto target 0
                       [0.5, 0, 0],       # label 5: d 0.5 from targets 0 and 1;    onto target 1
                       [5.0, 0, 0],       # label -1: a miss, d = 1;                does not move
                       [2.0, 0, 0],       # label -1: d 1 from target 1, a hit;     a NaN flow: bad AFTER only
                       [np.inf, 0, 0],    # label 7: bad on both sides
                       [9.0, 0, 0]],      # label 7: d 1 from target 2, a hit;      onto target 2
                      np.float32)
    flow = np.array([[-0.25, 0, 0], [0.5, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    labels = np.array([5, 5, -1, -1, 7, 7], np.float32)
    res = sr.residual(before, before, flow, labels, target, 1.0, (0.05, 0.5))
    assert res["labels"].tolist() == [-1.0, 5.0, 7.0] and res["rows"].tolist() == [2, 2, 2] and res["info"] == (1, 2, 1)
    assert res["idx_before"].tolist() == [0, 0, -1, 1, -2, 2] and res["idx_after"].tolist() == [0, 1, -1, -2, -2, 2]
    b, a = res["before"], res["after"]
    assert (b["rows"].tolist(), b["hits"].tolist(), b["under"].tolist()) == ([2, 2, 1], [1, 2, 1], [[0, 0], [0, 2], [0, 0]])
    assert (b["dsum"].tolist(), b["ddsum"].tolist()) == ([2.0, 0.75, 1.0], [2.0, 0.3125, 1.0])
    assert (a["rows"].tolist(), a["hits"].tolist(), a["under"].tolist()) == ([1, 2, 1], [0, 2, 1], [[0, 0], [2, 2], [1, 1]])
    assert (a["dsum"].tolist(), a["ddsum"].tolist()) == ([1.0, 0.0, 0.0], [1.0, 0.0, 0.0])
    t = sr.table18(res)
    assert t.shape == (3, 18)
    assert t[1].tolist() == [5, 2, 2, 2, 0, 2, 0, 0, 0.75, 0.3125, 2, 2, 2, 2, 0, 0, 0, 0]
    assert t[0].tolist() == [-1, 2, 2, 1, 0, 0, 0, 0, 2, 2, 1, 0, 0, 0, 0, 0, 1, 1]
    # the host-side class reads that table
    from icp_flow_amd import utils_eval
    s = utils_eval.SegmentResidual.from_table(t, (0.05, 0.5), 1.0, dict(bad_queries_before=1, bad_queries_after=2))
    assert s.labels.tolist() == [-1, 5, 7] and s.rows.tolist() == [2, 2, 2] and len(s) == 3
    assert s.before.mean(1) == 0.375 and s.after.mean(1) == 0.0 and s.gain().tolist() == [0.0, 0.375, 1.0]
    assert s.after.shares(1) == (1.0, 1.0) and s.before.hit_rate(0) == 0.5 and s.before.rms(2) == 1.0
    assert (s.before.bad, s.after.bad) == (1, 2)
    # both zeros are one label, NaN labels come last, one segment per bit pattern
    lab, L = cases.label_values()
    res = sr.residual(np.zeros((len(lab), 3)), np.zeros((len(lab), 3)), None, lab, target, 1.0, ())
    assert len(res["rows"]) == L and res["labels"][:5].tolist() == [-1e8, -1.0, 0.0, 3.0, 7.0] and math.isnan(res["labels"][5])
    assert res["rows"].tolist() == [2, 2, 4, 2, 1, 2] and not np.signbit(res["labels"][2])


def _hand_table():
    """seven segments of 10 rows; AFTER means: ground 0.5, noise 0.9, label 0 exactly 0.1, 3 and 4 both 0.3, 9 0.7, 12 no good row"""
    t = np.zeros((7, 18))
    t[:, 0] = [-1e8, -1.0, 0.0, 3.0, 4.0, 9.0, 12.0]
    t[:, 1] = 10
    t[:, 2] = t[:, 10] = [10, 10, 10, 10, 10, 10, 0]          # good rows on both sides
    t[:, 11] = [10, 10, 10, 5, 10, 0, 0]                       # hits AFTER
    t[:, 8] = [5.0, 9.0, 2.0, 1.0, 6.0, 7.0, 0.0]              # sum of d BEFORE
    t[:, 16] = [5.0, 9.0, 1.0, 3.0, 3.0, 7.0, 0.0]             # sum of d AFTER
    return t


def test_worst_orders_skips_and_looks_the_pair_up():
    from icp_flow_amd import utils_eval
    s = utils_eval.SegmentResidual.from_table(_hand_table(), (), 2.0)
    pairs = np.zeros((2, 10))
    pairs[0, :2], pairs[1, :2] = (9.0, 2.0), (3.0, 8.0)
    w = s.worst(pairs=pairs)
    # worst first; 3 and 4 tie at 0.3: ascending label; a mean of exactly 0.1 is not above 0.1; ground, noise and the
    # segment without a good row are not listed
    assert [e["label"] for e in w] == [9.0, 3.0, 4.0]
    assert [e["after_mean"] for e in w] == [0.7, 0.3, 0.3] and [e["before_mean"] for e in w] == [0.7, 0.1, 0.6]
    assert [e["gain"] for e in w] == [0.0, 0.1 - 0.3, 0.6 - 0.3] and [e["rows"] for e in w] == [10, 10, 10]
    assert [e["hit_rate_after"] for e in w] == [0.0, 0.5, 1.0]
    assert [e["matched"] for e in w] == [True, True, False] and [e["pair"] for e in w] == [[9.0, 2.0], [3.0, 8.0], None]
    assert list(w[0]) == ["label", "rows", "after_mean", "before_mean", "gain", "hit_rate_after", "matched", "pair"]
    assert [e["label"] for e in s.worst(pairs=torch.from_numpy(pairs))] == [9.0, 3.0, 4.0]
    assert [(e["matched"], e["pair"]) for e in s.worst()] == [(False, None)] * 3
    assert [e["label"] for e in s.worst(above=0.5)] == [9.0] and s.worst(above=0.7) == []
    assert [e["label"] for e in s.worst(above=0.05)] == [9.0, 3.0, 4.0, 0.0]
    assert [e["label"] for e in s.worst(skip=())] == [-1.0, 9.0, -1e8, 3.0, 4.0]
    assert [e["label"] for e in s.worst(skip=(9.0, 3.0))] == [-1.0, -1e8, 4.0]
    assert utils_eval.RESIDUAL_EDGES[1] == 0.1
    lines = utils_eval.format_segment_residual([dict(frame_pair=3, path="x", **e) for e in w])
    assert len(lines) == 3 and lines[0].startswith("residual segment: frame pair:    3,   9, after: 0.7000, before: 0.7000, gain: 0.0000, i:   9, j:   2;")
    assert "unmatched" in lines[2] and "len_i:     10" in lines[2]
    assert utils_eval.format_segment_residual(w)[1].startswith("residual segment:   3, after: 0.3000")


def _stub_register(args, fp, device):
    P = 2
    return dict(pairs=torch.zeros((P, 10)), transformations=torch.eye(4).repeat(P, 1, 1), flow=torch.from_numpy(fp.gt_flow.copy()))


def test_without_the_attribute_the_summary_has_todays_keys():
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=1, n_objects=3, n_max=60, n_background=50)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    s = frame_pairs.run_stream(frame_pairs.default_args(), [fp, fp], "cpu", register_fn=_stub_register)
    assert list(s) == ["frame_pairs", "matched_cluster_pairs", "n_gpus", "ms_per_frame_pair", "frame_pairs_per_s", "evaluated_points",
                       "pose_sources", "epe", "accs", "accr", "outlier", "Routlier"]
    # the attribute needs the residual's radius; with both, the work runs on the GPU only
    a = frame_pairs.default_args()
    a.residual_segments = True
    with pytest.raises(ValueError, match="needs args.residual"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    a.residual = 2.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    assert callable(frame_pairs.frame_segment_residual) and frame_pairs.RESIDUAL_SEGMENTS_SHOWN == 50


# ---- the conditions of the GPU tests' scenes ----------------------------------------------------------------------------------
def test_the_lattice_has_ties_and_hits_at_the_radius_on_both_sides():
    before, after, flow, labels, target, radius = cases.lattice()
    res = sr.residual(before, after, flow, labels, target, radius, cases.EDGES)
    r2 = rr.radius2(radius)
    q_after = after + flow
    for q, d2, idx in ((before, res["d2_before"], res["idx_before"]), (q_after, res["d2_after"], res["idx_after"])):
        at_radius = (d2 == r2) & (idx >= 0)
        assert at_radius.sum() == 150, "d2 == r2 must be a hit"
        D = ((q[:, None, :].astype(np.float64) - target[None, :, :]) ** 2).sum(axis=2)
        ties = ((D == D.min(axis=1, keepdims=True)).sum(axis=1) > 1) & (idx >= 0)
        assert ties.sum() > 100
        assert (idx[ties] == np.argmin(D[ties], axis=1)).all()                  # the lowest row
    assert (res["idx_before"] >= 0).all() and (res["idx_after"] >= 0).all() and len(res["rows"]) == 5


def test_the_bad_rows_are_bad_on_the_side_the_scene_says():
    before, after, flow, labels, target, inf_rows, pad_src, pad_dst = cases.one_side_bad()
    assert len(inf_rows) > 3 and len(pad_src) > 3 and len(pad_dst) > 3 and not set(inf_rows) & set(pad_src)
    res = sr.residual(before, after, flow, labels, target, 1.0, cases.EDGES)
    assert res["info"] == (len(pad_src), len(pad_src) + len(inf_rows), len(pad_dst))
    assert sorted(np.flatnonzero(res["idx_before"] == -2)) == sorted(pad_src)
    assert sorted(np.flatnonzero(res["idx_after"] == -2)) == sorted(set(pad_src) | set(inf_rows))
    assert int(res["before"]["rows"].sum()) == len(before) - len(pad_src)
    assert int(res["after"]["rows"].sum()) == len(before) - len(pad_src) - len(inf_rows)
    assert (res["before"]["rows"] > res["after"]["rows"]).any() and not np.isin(res["idx_after"], pad_dst).any()


def test_the_crowded_cell_is_one_cell():
    before, after, flow, labels, target, radius = cases.one_cell()
    cells = np.floor(target.astype(np.float64) / (1.01 * radius)).astype(int)
    assert len(target) == 5000 and (cells == 0).all()


def test_the_segment_sizes_straddle_the_wave_the_workgroup_and_the_chunk():
    assert set(cases.SEGMENT_SIZES) >= {1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 777}


def test_the_sabotaged_flow_spoils_one_segment_and_no_other():
    """the verdict's input: with (1, 0, 0) m added to one segment's flow that segment's AFTER mean exceeds 0.1 m and every other
    non-skipped segment stays below 1e-4 m; unsabotaged, every segment does"""
    for sabotage in (True, False):
        before, after, flow, labels, target = cases.verdict(sabotage=sabotage)
        res = sr.residual(before, after, flow, labels, target, 2.0, cases.EDGES)
        mean_after, mean_before = sr.means(res["after"]), sr.means(res["before"])
        seen = 0
        for c, label in enumerate(res["labels"].tolist()):
            if label in sr.SKIP:
                continue
            seen += 1
            if sabotage and label == cases.SABOTAGED:
                assert mean_after[c] > 0.1 and mean_after[c] > mean_before[c], (label, mean_after[c], mean_before[c])
            else:
                assert mean_after[c] < 1e-4, (label, mean_after[c])
        assert seen == 6 and cases.SABOTAGED in res["labels"].tolist() and {-1e8, -1.0} <= set(res["labels"].tolist())

"""CPU-only: the nearest-neighbour residual (icpflow_nn_residual, csrc/nnresid.hip; utils_eval.nn_residual; run_stream's
`--residual`) as far as it goes without a GPU -- the exports, every argument refusal with its code and message (all of them
come before any launch), the pinned size query, the command line, the host-side table, and the restatement the GPU tests
compare against (tests/residual_restatement.py) checked itself: against exact integer arithmetic on dyadic clouds and against
a scene counted by hand."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_restatement as rr        # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "workspace_sizes_nn_residual.json")
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib
    assert _lib.VERSION == 215
    for name, n_args in (("icpflow_nn_residual_workspace_bytes", 4), ("icpflow_nn_residual", 17)):
        assert hasattr(_lib._L, name) and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES["icpflow_nn_residual_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.NNR_MAX_GROUPS, _lib.NNR_MAX_EDGES) == (64, 4)
    hdr = open(os.path.join(REPO, "include", "icpflow_hip.h")).read()
    assert "#define ICPFLOW_NNR_MAX_GROUPS 64" in hdr and "#define ICPFLOW_NNR_MAX_EDGES 4" in hdr


def _call(**over):
    """icpflow_nn_residual with arguments that pass every check but the workspace's size (16 bytes: nothing is launched),
    `over` replacing some.  -> (status, message)"""
    from icp_flow_amd import _lib
    one = ctypes.c_void_p(4096)
    edges = np.asarray(over.pop("edges", (0.05, 0.1)), np.float64)
    a = dict(query=one, flow=None, n=10, target=one, m=10, radius=2.0, group=None, G=1,
             h_edges=edges.ctypes.data_as(ctypes.c_void_p) if len(edges) else None, E=len(edges), d2=one, idx=one, table=one, info=one,
             ws=one, ws_bytes=16)
    a.update(over)
    rc = _lib._L.icpflow_nn_residual(a["query"], a["flow"], a["n"], a["target"], a["m"], a["radius"], a["group"], a["G"], a["h_edges"], a["E"],
                                     a["d2"], a["idx"], a["table"], a["info"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    return rc, _lib._L.icpflow_last_error().decode()


def test_every_refusal_has_its_code_and_message():
    from icp_flow_amd import _lib
    # what passes every argument check stops at the workspace: the refusals below are not that one
    rc, msg = _call()
    assert rc == E_WORKSPACE and "icpflow_nn_residual_workspace_bytes" in msg
    rc, msg = _call(ws=None, ws_bytes=1 << 30)
    assert rc == E_WORKSPACE and "workspace" in msg
    for over in (dict(query=None), dict(target=None), dict(info=None), dict(h_edges=None)):
        rc, msg = _call(**over)
        assert rc == E_ARG and "null pointer" in msg, over
    # a cloud without rows needs no pointer
    assert _call(query=None, n=0)[0] == E_WORKSPACE and _call(target=None, m=0)[0] == E_WORKSPACE
    for over in (dict(n=-1), dict(m=-1)):
        rc, msg = _call(**over)
        assert rc == E_ARG and "< 0" in msg, over
    for r in (0.0, 0.99e-3, 1000.5, -2.0, float("nan"), float("inf")):
        rc, msg = _call(radius=r)
        assert rc == E_ARG and "radius" in msg and "[1e-3, 1e3]" in msg, r
    assert _call(radius=1e-3, edges=())[0] == E_WORKSPACE and _call(radius=1e3)[0] == E_WORKSPACE
    for G in (0, -1, 65, 1 << 20):
        rc, msg = _call(G=G)
        assert rc == E_ARG and "G must lie in [1, 64]" in msg, G
    assert _call(G=64)[0] == E_WORKSPACE
    rc, msg = _call(edges=(0.01, 0.02, 0.03, 0.04, 0.05))
    assert rc == E_ARG and "E must lie in [0, 4]" in msg
    rc, msg = _call(E=-1)
    assert rc == E_ARG and "E must lie in [0, 4]" in msg
    assert _call(edges=(0.01, 0.02, 0.03, 2.0))[0] == E_WORKSPACE and _call(edges=())[0] == E_WORKSPACE
    for edges in ((0.1, 0.05), (0.05, 0.05), (float("nan"), 0.1), (0.05, float("inf")), (0.05, 2.5), (0.0, 0.1), (-0.1, 0.1)):
        rc, msg = _call(edges=edges)
        assert rc == E_ARG and "edges must be finite, positive, strictly ascending and at most the radius" in msg, edges
    rc, msg = _call(d2=None, idx=None, table=None)
    assert rc == E_ARG and "all NULL" in msg
    for over in (dict(d2=None), dict(idx=None), dict(table=None), dict(d2=None, idx=None), dict(idx=None, table=None)):
        assert _call(**over)[0] == E_WORKSPACE, over
    for over in (dict(m=(1 << 29) + 1), dict(n=(1 << 29) + 1)):
        rc, msg = _call(**over)
        assert rc == E_LIMIT and "rows a cloud" in msg, over
    need = _lib._L.icpflow_nn_residual_workspace_bytes(10, 10, 1, 2)
    rc, msg = _call(ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    assert rc == E_ARG and "16-byte aligned" in msg


def _formula(n, m, G, E):
    """the size as include/icpflow_hip.h states it"""
    a = lambda x: -(-x // 256) * 256   # noqa: E731

    def table(k):
        H = 1
        while H < 2 * k:
            H *= 2
        return 2 * a(4 * H) + 4 * a(4 * -(-H // 1024)) + 256 + a(16 * k)

    grid = min(max(-(-n // 2048), 1), 256)
    return table(m) + table(n) + 2 * a(4 * n) + a(8 * grid * G * (E + 4))


def test_the_size_query_is_pinned_and_monotone():
    from icp_flow_amd import _lib
    q = _lib._L.icpflow_nn_residual_workspace_bytes
    recorded = json.load(open(GOLDEN))["icpflow_nn_residual_workspace_bytes"]
    assert len(recorded) >= 100
    for n, m, G, E, size in recorded:
        assert q(n, m, G, E) == size == _formula(n, m, G, E) and size % 256 == 0 and size > 0, (n, m, G, E)
    sizes = [0, 1, 63, 64, 65, 511, 512, 513, 2049, 20000, 63276, 130000, 1 << 20]
    for G, E in ((1, 0), (4, 2), (64, 4)):
        for m in sizes:
            by_n = [q(n, m, G, E) for n in sizes]
            assert by_n == sorted(by_n), (m, G, E)
        for n in sizes:
            by_m = [q(n, m, G, E) for m in sizes]
            assert by_m == sorted(by_m), (n, G, E)
    # arguments the call refuses
    assert q(-1, 1, 1, 0) == 0 and q(1, -1, 1, 0) == 0 and q(1, 1, 0, 0) == 0 and q(1, 1, 65, 0) == 0 and q(1, 1, 1, 5) == 0
    assert q(1, (1 << 29) + 1, 1, 0) == 0 and q((1 << 29) + 1, 1, 1, 0) == 0


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_eval
    x = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.nn_residual(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.chamfer(x, x, 2.0)


def test_the_flag_parses_bare_and_with_a_value():
    from icp_flow_amd import frame_pairs
    ap = frame_pairs.argument_parser()
    assert ap.parse_args(["dir"]).residual is None
    assert ap.parse_args(["dir", "--residual"]).residual == 2.0
    assert ap.parse_args(["dir", "--residual", "0.5"]).residual == 0.5
    assert ap.parse_args(["--residual", "0.25", "dir", "--in-flight", "4"]).residual == 0.25
    with pytest.raises(SystemExit, match="--residual is not built into --protocol reference"):
        frame_pairs.main(["dir", "--residual", "--protocol", "reference"])


def test_the_restatement_equals_exact_integer_arithmetic():
    """several hundred dyadic clouds -- duplicates, lattices with queries half way between points, the edge of the range --
    where every float32 operation of the statement is exact: d2 must be the int64 computation and idx the first minimum"""
    scenes = rr.dyadic_clouds(400, seed=11)
    hits = ties = 0
    for kq, kf, kt, radius in scenes:
        q, f, t = rr.dyadic_floats(kq, kf, kt)
        d2, idx, info = rr.search(q.reshape(-1, 3), t.reshape(-1, 3), f, radius)
        want_d2, want_idx = rr.exact_dyadic(kq, kf, kt, radius)
        assert np.array_equal(d2, want_d2) and np.array_equal(idx, want_idx), (len(kq), len(kt), radius)
        assert info == dict(bad_queries=0, bad_targets=0)
        hits += int((idx >= 0).sum())
        if len(kt):
            D = (((kq + (0 if kf is None else kf))[:, None, :] - kt[None, :, :]) ** 2).sum(axis=2)
            ties += int(((D == D.min(axis=1, keepdims=True)).sum(axis=1) > 1)[idx >= 0].sum())
    assert hits > 2000 and ties > 300          # (the scenes do exercise hits and the lowest-row rule)


def test_a_scene_counted_by_hand():
    """three groups, two edges, radius 1: targets on the x axis; every number below is worked out by hand"""
    target = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [1e8, 1e8, 1e8], [10, 0, 0]], np.float32)
    query = np.array([[0.0, 0, 0],        # on target 0: d 0
                      [0.5, 0, 0],        # half way between 0 and 1: d 0.5 from both, the lowest row (0) wins
                      [1.0, 0.03, 0],     # next to the duplicated targets 1 and 2: row 1, d 0.03
                      [2.0, 0, 0],        # d 1 from target 1: d2 == r2 is a hit
                      [5.0, 0, 0],        # nothing within 1 m: a miss, d = 1
                      [9.0, 0.08, 0],     # flow (1, 0, 0) takes it to (10, 0.08, 0): row 5, d 0.08
                      [np.inf, 0, 0],     # a bad row
                      [0.0, 0, 0],        # group 3 of G = 3: a bad row
                      [0.25, 0, 0]],      # d 0.25 from target 0
                     np.float32)
    flow = np.zeros_like(query)
    flow[5, 0] = 1.0
    groups = np.array([0, 0, 1, 1, 1, 2, 0, 3, 2], np.int32)
    edges = (0.05, 0.5)
    d2, idx, tab, info = rr.residual(query, target, flow, 1.0, groups, 3, edges)
    f32 = np.float32
    assert idx.tolist() == [0, 0, 1, 1, -1, 5, -2, -2, 0]
    assert d2.tolist() == [0.0, 0.25, float(f32(0.03) * f32(0.03)), 1.0, 1.0, float(f32(0.08) * f32(0.08)), 1.0, 1.0, 0.0625]
    assert info == dict(bad_queries=2, bad_targets=2)
    assert tab["rows"].tolist() == [2, 3, 2] and tab["hits"].tolist() == [2, 2, 2]
    assert tab["under"].tolist() == [[1, 2], [1, 1], [0, 2]]
    d = lambda v: float(np.sqrt(f32(v)))   # noqa: E731
    d03, d08 = d(f32(0.03) * f32(0.03)), d(f32(0.08) * f32(0.08))
    assert tab["dsum"].tolist() == [0.5, math.fsum([d03, 1.0, 1.0]), math.fsum([d08, 0.25])]
    assert tab["ddsum"].tolist() == [0.25, math.fsum([d03 * d03, 1.0, 1.0]), math.fsum([d08 * d08, 0.0625])]
    # the next float32 above r2 is a miss
    over = np.array([[np.nextafter(f32(2.0), f32(3.0)), 0, 0]], np.float32)
    d2o, idxo, _ = rr.search(over, target, None, 1.0)
    assert idxo.tolist() == [-1] and d2o.tolist() == [1.0]
    # no targets at all: every good query is a miss
    d2e, idxe, _ = rr.search(query, np.zeros((0, 3), np.float32), flow, 1.0, groups, 3)
    assert idxe.tolist() == [-1, -1, -1, -1, -1, -1, -2, -2, -1] and (d2e == 1.0).all()


def test_the_table_adds_and_round_trips_exactly():
    from icp_flow_amd import utils_eval
    rng = np.random.default_rng(5)
    tabs = []
    for k in range(3):
        n = 200
        d2 = (rng.uniform(0, 2.0, n).astype(np.float32)) ** 2
        idx = rng.integers(-2, 50, n).astype(np.int32)
        groups = rng.integers(0, 4, n)
        tabs.append(rr.table(d2, idx, groups, 4, utils_eval.RESIDUAL_EDGES))
    words = [rr.table_words(t) for t in tabs]
    ts = [utils_eval.ResidualTable.from_words(w, 4, utils_eval.RESIDUAL_EDGES, 2.0, bad=k) for k, w in enumerate(words)]
    for t, w, tab in zip(ts, words, tabs):
        assert np.array_equal(t.words(), w) and t.words().dtype == np.int64
        assert np.array_equal(t.rows, tab["rows"]) and np.array_equal(t.under, tab["under"]) and np.array_equal(t.dsum, tab["dsum"])
    total = utils_eval.ResidualTable.zeros(4, utils_eval.RESIDUAL_EDGES, 2.0)
    for t in ts:
        assert total.add(t) is total
    assert np.array_equal(total.rows, sum(t["rows"] for t in tabs)) and np.array_equal(total.hits, sum(t["hits"] for t in tabs))
    assert np.array_equal(total.under, sum(t["under"] for t in tabs)) and total.bad == 3
    assert np.array_equal(total.dsum, (tabs[0]["dsum"] + tabs[1]["dsum"]) + tabs[2]["dsum"])          # in call order
    assert np.array_equal(total.ddsum, (tabs[0]["ddsum"] + tabs[1]["ddsum"]) + tabs[2]["ddsum"])
    back = utils_eval.ResidualTable.from_words(total.words(), 4, utils_eval.RESIDUAL_EDGES, 2.0)
    assert np.array_equal(back.words(), total.words())
    g = 2
    assert total.n(g) == int(total.rows[g]) and total.n() == int(total.rows.sum())
    assert total.mean(g) == total.dsum[g] / total.rows[g] and total.rms(g) == math.sqrt(total.ddsum[g] / total.rows[g])
    assert total.hit_rate(g) == total.hits[g] / total.rows[g]
    assert total.shares(g) == tuple(total.under[g] / total.rows[g])
    empty = utils_eval.ResidualTable.zeros(2, (), 1.0)
    assert math.isnan(empty.mean(0)) and math.isnan(empty.rms()) and empty.shares() == ()
    with pytest.raises(ValueError):
        total.add(empty)
    text = utils_eval.format_residual(dict(forward=ts[0], backward=ts[1]), dict(forward=ts[2], backward=ts[1]))
    assert "matched" in text and "Chamfer" in text and f"{ts[0].mean(3):.6f} -> {ts[2].mean(3):.6f}" in text


def _stub_register(args, fp, device):
    P = 2
    return dict(pairs=torch.zeros((P, 10)), transformations=torch.eye(4).repeat(P, 1, 1), flow=torch.from_numpy(fp.gt_flow.copy()))


def test_without_the_flag_the_summary_has_todays_keys():
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=1, n_objects=3, n_max=60, n_background=50)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    s = frame_pairs.run_stream(frame_pairs.default_args(), [fp, fp], "cpu", register_fn=_stub_register)
    assert list(s) == ["frame_pairs", "matched_cluster_pairs", "n_gpus", "ms_per_frame_pair", "frame_pairs_per_s", "evaluated_points",
                       "pose_sources", "epe", "accs", "accr", "outlier", "Routlier"]
    assert (s["frame_pairs"], s["matched_cluster_pairs"], s["epe"]) == (2, 4, 0.0)
    bare = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"])
    s = frame_pairs.run_stream(frame_pairs.default_args(), [bare], "cpu", register_fn=lambda a, f, dev: _stub_register(a, fp, dev))
    assert list(s) == ["frame_pairs", "matched_cluster_pairs", "n_gpus", "ms_per_frame_pair", "frame_pairs_per_s", "evaluated_points",
                       "pose_sources"]
    # with the flag the residual runs on the GPU only
    a = frame_pairs.default_args()
    a.residual = 2.0
    with pytest.raises(RuntimeError, match="no CPU path"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)


def test_the_groups_of_the_source_rows():
    from icp_flow_amd import frame_pairs
    labels = torch.tensor([-1e8, -1.0, 0.0, 1.0, 2.0, 2.0, 7.0, -1.0], dtype=torch.float32)
    pairs = torch.zeros((2, 10))
    pairs[0, 0], pairs[1, 0] = 2.0, 7.0
    assert frame_pairs.residual_groups(labels, pairs).tolist() == [0, 1, 2, 2, 3, 3, 3, 1]
    assert frame_pairs.residual_groups(labels, torch.zeros((0, 10))).tolist() == [0, 1, 2, 2, 2, 2, 2, 1]
    assert frame_pairs.residual_groups(labels, pairs).dtype == torch.int32

"""CPU-only: the track repair (icpflow_object_tracks_suspects, icpflow_pairs_repair_select, icpflow_pairs_reregister;
csrc/tracks.hip, csrc/repair.hip; utils_tracks, pair_judges.frame_tracks(repair=True), --tracks-repair).  The exports and their
refusals (no GPU is needed for a refusal), the workspace formula, the flag, the numpy restatement (tests/repair_restatement.py)
on hand-made tables and against np.linalg.lstsq, every reason of the select on thresholds hit exactly, and the end-to-end scene
under the oracle alone."""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repair_cases as rc                     # noqa: E402
import repair_restatement as rr               # noqa: E402

F = np.float32
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes_pairs_reregister.json")


@pytest.fixture(autouse=True)
def feature():
    """every test below speaks about a library that has the repair: without its exports none of them passes"""
    from icp_flow_amd import _lib, pair_judges
    assert all(hasattr(_lib._L, name) for name in ("icpflow_object_tracks_suspects", "icpflow_pairs_repair_select", "icpflow_pairs_reregister"))
    assert "repair" in pair_judges.frame_tracks.__code__.co_varnames


def _lib_and_fakes():
    from icp_flow_amd import _lib
    return _lib, _lib._L, ctypes.c_void_p(4096)


# --------------------------------------------------------------------------------------------------------------------------- ABI

def test_the_exports_exist_the_structs_match_and_the_defaults_hold():
    from icp_flow_amd import _lib, build
    assert "repair.hip" in build.SOURCES and "rejecttest.hpp" in build.HEADERS
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "icpflow_hip.h")).read()
    for name in ("icpflow_object_tracks_suspects", "icpflow_pairs_repair_default_params", "icpflow_pairs_repair_select",
                 "icpflow_pairs_reregister_workspace_bytes", "icpflow_pairs_reregister"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(_lib._L, name)
    assert "8(m)  track repair" in hdr and _lib.VERSION == 215
    for define, value in (("ICPFLOW_TRACK_PLAN_COLS", 8), ("ICPFLOW_TRACK_PLAN_COUNTS", 4), ("ICPFLOW_REPAIR_COLS", 12), ("ICPFLOW_REPAIR_COUNTS", 8)):
        assert f"#define {define} {value}\n" in hdr
    assert (_lib.TRACK_PLAN_COLS, _lib.TRACK_PLAN_COUNTS, _lib.REPAIR_COLS, _lib.REPAIR_COUNTS) == (rr.PLAN_COLS, rr.PLAN_COUNTS, rr.REPAIR_COLS, rr.REPAIR_COUNTS)
    p = _lib.RepairParams.defaults()
    assert ctypes.sizeof(_lib.RepairParams) == 48 and p.struct_size == 48
    assert p.as_dict() == rr.DEFAULTS == dict(translation_frame=2.0, thres_iou=0.2, rot_limit_deg=9.0, thres_error=0.2, max_residual=0.2)
    with pytest.raises(TypeError):
        _lib.RepairParams.defaults(struct_size=1)
    assert _lib._L.icpflow_pairs_repair_default_params(None) == E_ARG


def test_the_plan_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackParams.defaults()

    def call(**over):
        a = dict(obs=one, M=5, T=3, params=good, plan=one, counts=one)
        a.update(over)
        rc_ = L.icpflow_object_tracks_suspects(a["obs"], a["M"], a["T"], ctypes.byref(a["params"]) if a["params"] is not None else None, a["plan"], a["counts"], None)
        return rc_, L.icpflow_last_error().decode()

    short = _lib.TrackParams.defaults()
    short.struct_size = 8
    for over, code, text in ((dict(M=-1), E_ARG, "negative"), (dict(T=-1), E_ARG, "negative"), (dict(M=(1 << 16) + 1), E_LIMIT, "at most"),
                             (dict(T=(1 << 24) + 1), E_LIMIT, "at most"), (dict(obs=None), E_ARG, "null pointer"), (dict(plan=None), E_ARG, "null pointer"),
                             (dict(counts=None), E_ARG, "null pointer"), (dict(params=None), E_ARG, "null pointer"), (dict(params=short), E_ARG, "struct_size"),
                             (dict(params=_lib.TrackParams.defaults(max_residual=float("nan"))), E_ARG, "max_residual"),
                             (dict(params=_lib.TrackParams.defaults(max_residual=-0.5)), E_ARG, "max_residual"),
                             (dict(params=_lib.TrackParams.defaults(max_residual=float("inf"))), E_ARG, "max_residual")):
        got, msg = call(**over)
        assert got == code and text in msg and msg.startswith("icpflow_object_tracks_suspects"), (over, got, msg)


SELECT_POINTERS = ("T_new", "T_old", "iters", "errors", "ious", "translations", "rotations", "errors_old", "centre", "pred", "T_out", "report", "counts")


def test_the_select_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.RepairParams.defaults()

    def call(**over):
        a = dict({k: one for k in SELECT_POINTERS}, K=3, params=good)
        a.update(over)
        rc_ = L.icpflow_pairs_repair_select(a["T_new"], a["T_old"], a["iters"], a["errors"], a["ious"], a["translations"], a["rotations"], a["errors_old"],
                                            a["centre"], a["pred"], a["K"], ctypes.byref(a["params"]) if a["params"] is not None else None, a["T_out"],
                                            a["report"], a["counts"], None)
        return rc_, L.icpflow_last_error().decode()

    short = _lib.RepairParams.defaults()
    short.struct_size = 40
    cases = [(dict(K=-1), E_ARG, "negative"), (dict(K=(1 << 24) + 1), E_LIMIT, "at most"), (dict(params=None), E_ARG, "null pointer"),
             (dict(params=short), E_ARG, "struct_size")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in SELECT_POINTERS]
    for name in ("translation_frame", "thres_iou", "rot_limit_deg", "thres_error", "max_residual"):
        cases += [(dict(params=_lib.RepairParams.defaults(**{name: bad})), E_ARG, name) for bad in (-1.0, float("nan"), float("inf"))]
    for over, code, text in cases:
        got, msg = call(**over)
        assert got == code and text in msg and msg.startswith("icpflow_pairs_repair_select"), (over, got, msg)


def test_the_reregistration_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.RepairParams.defaults()
    tables = _lib.Tables(4096, 4096, 4096, 4096, 4096, 4096, 4, 4, 9)
    pointers = ("seg", "clouds", "init", "T_old", "centre", "pred", "T_out", "report", "counts")

    def reg(**over):
        r = dict(thres_dist=0.1, rel=1e-6, max_it=100, stop=0)
        r.update(over)
        return _lib.Registration(None, None, None, 0, 0, 0, 0.0, r["thres_dist"], r["rel"], r["max_it"], r["stop"])

    def call(**over):
        a = dict({k: one for k in pointers}, tables=tables, K=3, N=256, reg=reg(), params=good, ws=one, ws_bytes=1 << 30)
        a.update(over)
        ref = lambda x: ctypes.byref(x) if x is not None else None     # noqa: E731
        rc_ = L.icpflow_pairs_reregister(ref(a["tables"]), a["K"], a["N"], a["seg"], a["clouds"], a["init"], a["T_old"], a["centre"], a["pred"], ref(a["reg"]),
                                         ref(a["params"]), a["T_out"], a["report"], a["counts"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None, None)
        return rc_, L.icpflow_last_error().decode()

    short = _lib.RepairParams.defaults()
    short.struct_size = 8
    need = int(L.icpflow_pairs_reregister_workspace_bytes(3, 256))
    assert need > 0
    cases = [(dict(K=-1), E_ARG, "negative"), (dict(N=0), E_ARG, "N must be"), (dict(K=1 << 16, N=(1 << 14) + 1), E_LIMIT, "at most"),
             (dict(tables=None), E_ARG, "null pointer"), (dict(tables=_lib.Tables(None, 4096, 4096, 4096, 4096, 4096, 4, 4, 9)), E_ARG, "null pointer"),
             (dict(reg=None), E_ARG, "null pointer"), (dict(params=None), E_ARG, "null pointer"), (dict(params=short), E_ARG, "struct_size"),
             (dict(params=_lib.RepairParams.defaults(max_residual=-1.0)), E_ARG, "max_residual"),
             (dict(params=_lib.RepairParams.defaults(thres_error=float("nan"))), E_ARG, "thres_error"),
             (dict(reg=reg(max_it=0)), E_ARG, "max_iterations"), (dict(reg=reg(max_it=1025)), E_ARG, "max_iterations"), (dict(reg=reg(stop=2)), E_ARG, "stop_mode"),
             (dict(reg=reg(thres_dist=float("nan"))), E_ARG, "thres_dist"),
             (dict(ws=None), E_WORKSPACE, "icpflow_pairs_reregister_workspace_bytes"), (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"),
             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in pointers]
    for over, code, text in cases:
        got, msg = call(**over)
        assert got == code and text in msg and msg.startswith("icpflow_pairs_reregister"), (over, got, msg)


def test_the_workspace_formula_equals_the_golden_file_and_never_shrinks():
    _lib, L, _ = _lib_and_fakes()
    fn = L.icpflow_pairs_reregister_workspace_bytes
    a256 = lambda b: (b + 255) // 256 * 256     # noqa: E731
    golden = json.load(open(GOLDEN))
    assert len(golden["sizes"]) >= 12
    for K, N, want in golden["sizes"]:
        assert int(fn(K, N)) == want == a256(4 * (44 * K + 1)) + a256(_lib.workspace_bytes(K, N)), (K, N, int(fn(K, N)), want)
    Ks, Ns = [1, 2, 3, 17, 63, 64, 65, 257, 1024], [1, 64, 256, 600, 1024, 1025, 1100, 2048, 10000]
    for K in Ks:
        sizes = [int(fn(K, N)) for N in Ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes), (K, sizes)
    for N in Ns:
        sizes = [int(fn(K, N)) for K in Ks]
        assert sizes == sorted(sizes), (N, sizes)
    assert fn(-1, 64) == 0 and fn(0, 64) == 0 and fn(4, 0) == 0 and fn(1 << 16, (1 << 14) + 1) == 0


# ---------------------------------------------------------------------------------------------------------------- the flag

def test_the_flag_goes_with_tracks_and_the_defaults_stay():
    from icp_flow_amd import frame_pairs
    ns = frame_pairs.argument_parser().parse_args(["dir"])
    assert ns.tracks_repair is False
    assert frame_pairs.argument_parser().parse_args(["dir", "--tracks", "--tracks-repair"]).tracks_repair is True
    with pytest.raises(SystemExit, match="--tracks-repair goes with --tracks"):
        frame_pairs.main(["dir", "--tracks-repair"])
    with pytest.raises(SystemExit, match="--tracks-repair goes with --tracks"):
        frame_pairs.main(["dir", "--tracks-repair", "--tracks-log"])
    with pytest.raises(SystemExit, match="--tracks is not built into --protocol reference"):
        frame_pairs.main(["dir", "--tracks", "--tracks-repair", "--protocol", "reference"])
    with pytest.raises(SystemExit, match="--tracks-min-iou"):
        frame_pairs.main(["dir", "--tracks", "--tracks-repair", "--tracks-min-iou", "0"])
    assert "tracks_repair" not in frame_pairs.DEFAULT_ARGS and not hasattr(frame_pairs.default_args(), "tracks_repair")
    assert frame_pairs.DEFAULT_ARGS["max_points"] == 10000 and frame_pairs.DEFAULT_ARGS["thres_error"] == 0.2
    a = frame_pairs.default_args()
    a.tracks_repair = True
    with pytest.raises(ValueError, match="args.tracks_repair goes with args.tracks"):
        frame_pairs.run_stream(a, [], "cpu")
    a.tracks = True
    with pytest.raises(ValueError, match="args.tracks under more than one rank"):
        frame_pairs.run_stream(a, [], "cpu", rank=0, world=2)


def test_the_repair_report_sums_into_a_summary():
    from icp_flow_amd import utils_tracks
    assert utils_tracks.REPAIR_REASONS[rr.TOO_LONG] == "too_long" and len(utils_tracks.REPAIR_REASONS) == 7 and utils_tracks.REPAIR_TOO_LONG == rr.TOO_LONG
    tracks = lambda consistent: SimpleNamespace(fit_counts=np.array([5, 5, 5, consistent, 4]))     # noqa: E731
    done = utils_tracks.Repair(tracks(3), [15, 15, 3, 2], [dict(gap=1, pair=0)], [1, 0, 0, 0, 1, 0, 1, 0], ms=2.5)
    assert done.summary(tracks(4)) == dict(suspects=2, retried=2, accepted=1, consistent_before=3, consistent_after=4,
                                           reasons=dict(accepted=1, reject_test=0, error=0, off_prediction=0, not_better=1, abandoned=0, too_long=1))
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.suspects_device(torch.zeros((2, 13), dtype=torch.float64), 1)


# --------------------------------------------------------------------------------------------------------------------- the plan

def test_three_gaps_with_one_outlier_name_exactly_that_row():
    plan, counts = rr.plan(rc.one_outlier(bad=2), 1)
    assert plan[:, 0].tolist() == [0, 1, 0] and counts.tolist() == [3, 3, 1, 1]
    assert plan[1, 1:3].tolist() == [2, 2] and plan[1, 3:6].tolist() == [0.5, -0.25, 0.0625] and plan[1, 6] == 1.0 and plan[1, 7] == 0.0
    assert (plan[[0, 2], 7] > 0.2).all()                                     # with the outlier among the others they do not agree
    for bad in (1, 3):
        assert rr.plan(rc.one_outlier(bad=bad), 1)[0][:, 0].tolist() == [float(g == bad) for g in (1, 2, 3)]


def test_two_outliers_of_three_name_none():
    rows = rc.one_outlier(bad=2)
    rows[2][4] -= 1.0                                                         # gap 3 leaves the line too, the other way
    plan, counts = rr.plan(rows, 1)
    assert not plan[:, 0].any() and counts.tolist() == [3, 3, 0, 0]


def test_two_gaps_only_leave_no_row_eligible():
    plan, counts = rr.plan(rc.one_outlier(gaps=(1, 2), bad=2), 1)
    assert counts.tolist() == [2, 0, 0, 0] and plan[:, 1:3].tolist() == [[1, 1], [1, 1]] and not plan[:, [0, 3, 4, 5, 6, 7]].any()


def test_two_observations_in_one_gap_count_as_one_distinct_gap():
    rows = rc.one_outlier(gaps=(1, 2), bad=0) + [rc.obs(0, 2, 0.25, (0.5, -0.25, 0.0625))]
    plan, counts = rr.plan(rows, 1)
    assert plan[:, 1].tolist() == [2, 2, 2] and plan[:, 2].tolist() == [1, 2, 2] and counts.tolist() == [3, 2, 2, 0]
    assert not plan[0, [0, 3, 4, 5, 6, 7]].any()                             # two others, both of gap 2: not eligible
    far = rr.plan(rc.one_outlier() + [rc.obs(0, 64, 0.5, (9.0, 9.0, 9.0)), rc.obs(0, -1, 0.5, (9.0, 9.0, 9.0))], 1)[0]
    assert far[0, 1:3].tolist() == [4, 2]                                    # gaps outside [0, 63] are rows but set no bit
    skipped, counts = rr.plan([rc.obs(-1, 1, 0.1, (1, 1, 1)), rc.obs(1, 1, 0.1, (1, 1, 1)), rc.obs(np.nan, 1, 0.1, (1, 1, 1))], 1)
    assert not skipped.any() and counts.tolist() == [0, 0, 0, 0]


def test_r2_exactly_m2_is_not_suspect_and_inner_exactly_m2_is_still_consistent():
    # the others on a line through the origin, this gap 0.25 beside it: r2 = 0.0625 = m2 exactly
    on = lambda off: [rc.obs(0, 1, 0.125, (0.25, 0.0, 0.0)), rc.obs(0, 2, 0.25, (0.5, off, 0.0)), rc.obs(0, 3, 0.375, (0.75, 0.0, 0.0))]   # noqa: E731
    plan, _ = rr.plan(on(0.25), 1, max_residual=0.25)
    assert plan[1, 6] == 0.25 and plan[1, 0] == 0.0
    plan, _ = rr.plan(on(float(np.nextafter(0.25, 1.0))), 1, max_residual=0.25)
    assert plan[1, 0] == 1.0
    # the others: s = 0.5 each, d = (0, +-0.25): v = 0, inner = 0.0625 = m2 exactly -- they still agree
    rows = lambda y: [rc.obs(0, 1, 0.5, (0.0, y, 0.0)), rc.obs(0, 2, 0.5, (0.0, -y, 0.0)), rc.obs(0, 3, 0.5, (4.0, 0.0, 0.0))]   # noqa: E731
    plan, counts = rr.plan(rows(0.25), 1, max_residual=0.25)
    assert plan[2, 7] == 0.25 and plan[2, 0] == 1.0 and counts[2] == 1
    plan, counts = rr.plan(rows(float(np.nextafter(0.25, 1.0))), 1, max_residual=0.25)
    assert plan[2, 0] == 0.0 and counts[2] == 0 and counts[1] == 3


def test_the_leave_one_out_velocity_equals_least_squares_through_the_origin():
    """p = s_j v with v = (sum s d) / (sum s s) over the K other rows: as tests/test_tracks.py derives for the fit,
    |v - v_exact| <= (2 K + 3) u sum|s d| / sum s s to first order, u = 2^-53, and 16 u |d| / |s| is allowed for np.linalg.lstsq's own
    error; the product s_j v adds one rounding, u |s_j v|."""
    rng = np.random.default_rng(8)
    u = 2.0 ** -53
    for K in (2, 3, 8):
        for _ in range(20):
            s = 0.1 * rng.integers(1, 16, K + 1)
            d = s[:, None] * rng.normal(0, 5, 3) + rng.normal(0, 0.05, (K + 1, 3))
            plan, _ = rr.plan([rc.obs(0, g, s[g], d[g]) for g in range(K + 1)], 1)
            for j in range(K + 1):
                rest = np.arange(K + 1) != j
                want = np.linalg.lstsq(s[rest, None], d[rest], rcond=None)[0][0]
                for a in range(3):
                    bound = (2 * K + 3) * u * np.abs(s[rest] * d[rest, a]).sum() / (s[rest] ** 2).sum() + 16 * u * np.linalg.norm(d[rest, a]) / np.linalg.norm(s[rest])
                    assert abs(plan[j, 3 + a] - s[j] * want[a]) <= s[j] * bound + u * abs(s[j] * want[a]), (K, j, a)


def test_the_random_tables_reach_every_kind_of_row():
    seen = np.zeros(4, np.int64)
    for obs, T in rc.random_tables(60):
        plan, counts = rr.plan(obs, T)
        assert counts[0] >= counts[1] >= counts[2] >= counts[3] and counts[3] == plan[:, 0].sum()
        seen += counts
    assert (seen > 0).all()


# ------------------------------------------------------------------------------------------------------------------- the select

def test_every_reason_is_reached_on_its_threshold():
    rows, want = rc.threshold_rows()
    T_out, report, counts = rr.select(iters=7, **rc.stack(rows), **rc.PARAMS)
    assert report[:, 0].tolist() == want and set(want) == {0, 1, 2, 3, 4}
    assert counts.tolist() == [want.count(r) for r in range(6)] + [0, 0]
    table = rc.stack(rows)
    for k, reason in enumerate(want):
        assert T_out[k].tobytes() == (table["T_new"] if reason == 0 else table["T_old"])[k].tobytes()
        assert report[k, 11] == float(reason == 0) and report[k, 7] == 7
    abandoned = rr.select(iters=-1, **table, **rc.PARAMS)
    assert abandoned[2].tolist() == [0, 0, 0, 0, 0, len(rows), 0, 0] and abandoned[0].tobytes() == table["T_old"].tobytes()


def test_one_float32_step_either_side_of_thres_error_and_an_equal_error_decide_as_stated():
    te = F(0.2)
    for e, reason in ((np.nextafter(te, F(0)), 0), (te, 2), (np.nextafter(te, F(1)), 2)):
        got = rr.select(iters=1, **rc.stack([rc.select_row(errors=(e, 0.9), errors_old=(0.9, 0.9))]))
        assert got[1][0, 0] == reason and got[1][0, 1] == float(e)
    # 0.2 as a double lies below float32(0.2): compared in float32 the threshold itself is not below it, in fp64 it would be
    assert float(te) > 0.2
    same = rr.select(iters=1, **rc.stack([rc.select_row(errors=(0.07, 0.05), errors_old=(0.05, 0.08))]))
    assert same[1][0, :3].tolist() == [0, float(F(0.05)), float(F(0.05))]
    worse = rr.select(iters=1, **rc.stack([rc.select_row(errors=(0.07, 0.05), errors_old=(np.nextafter(F(0.05), F(0)), 0.08))]))
    assert worse[1][0, 0] == 4


def test_nans_go_where_the_header_says():
    nan = np.nan
    row = lambda **over: rr.select(iters=1, **rc.stack([rc.select_row(**over)]))[1][0]     # noqa: E731
    assert row(errors=(nan, 0.01))[0] == 2 and np.isnan(row(errors=(nan, 0.01))[1])        # e_new NaN if either error is
    assert row(errors_old=(nan, 0.001))[0] == 0 and np.isnan(row(errors_old=(nan, 0.001))[2])   # a NaN e_old is +inf: accepted
    assert row(translations=(nan, 0, 0))[0] == 0 and np.isnan(row(translations=(nan, 0, 0))[9])  # a NaN passes the test it sits in
    assert row(ious=(nan, 0.0))[0] == 0 and row(ious=(0.0, nan))[0] == 1                   # Python's min on the two-element tensor
    assert row(rotations=(0, nan, 80.0))[0] == 0 and row(rotations=(0, nan, 80.0))[10] == 80.0
    gone = row(T_new=rc.translation((nan, nan, nan)))
    assert gone[0] == 0 and np.isnan(gone[3:7]).all()                                      # (an abandoned batch is caught by its count)


# --------------------------------------------------------------------------------------------------------------- the bookkeeping

def test_the_patch_changes_the_accepted_pairs_and_nothing_else():
    rng = np.random.default_rng(2)
    pairs = np.concatenate([np.array([[3, 5], [4, 6], [7, 8]], F), rng.random((3, 8)).astype(F)], axis=1)
    T = np.tile(np.eye(4, dtype=F), (3, 1, 1))
    labels = np.array([3, 3, 4, 7, -1, 4, 9], F)
    T_out = np.stack([rc.translation((1, 0, 0)), rc.IDENTITY])
    report = np.zeros((2, 12))
    report[0, 11] = 1.0
    metrics = {k: np.full((2, 2), 10.0 + c, F) for c, k in enumerate(("errors", "inliers", "ratios", "ious"))}
    got_pairs, got_T, changed = rr.patch(pairs, T, labels, [1, 2], T_out, report, metrics)
    assert changed.tolist() == [False, False, True, False, False, True, False]
    assert got_pairs[1].tolist() == [4, 6, 10, 10, 11, 11, 12, 12, 13, 13] and np.array_equal(got_pairs[[0, 2]], pairs[[0, 2]])
    assert got_T[1, 0, 3] == 1.0 and np.array_equal(got_T[[0, 2]], T[[0, 2]])


# --------------------------------------------------------------------------------------------------------------------- the scene

def test_the_scene_is_what_the_end_to_end_test_claims_under_the_oracle():
    """Under the oracle alone: its CPU DBSCAN gives one cluster per object in every gap; its apply_icp from [I | p] on the pair a
    test writes the fault into lands within max_residual of the truth, and the restated select accepts it over the faulted pose;
    on the box that truly leaves its line the slid pose passes the association's reject test and the error threshold, lies on
    the prediction, and is refused because its min(error) is larger than the registered pose's."""
    import torch
    from oracle import cluster as oc
    from oracle import reference_path as rp
    sc = rc.scene()
    raw, t, obj = sc["arrays"]["raw_points"].astype(np.float64), sc["arrays"]["time_indice"], sc["object"]
    a = SimpleNamespace(epsilon=rc.CLUSTER["epsilon"], min_cluster_size=rc.CLUSTER["min_cluster_size"], num_clusters=rc.CLUSTER["num_clusters"])
    for j in range(1, rc.FRAMES):
        rows = np.concatenate([np.flatnonzero(t == 0), np.flatnonzero(t == j)])          # dst first, as cluster_frame_pair stacks them
        labels = oc.cluster_pcd(a, raw[rows], np.ones(len(rows), bool))
        for side in (slice(0, int((t == 0).sum())), slice(int((t == 0).sum()), None)):
            seen = [set(labels[side][obj[rows][side] == k].tolist()) for k in range(len(rc.STEPS))]
            assert all(len(s) == 1 and min(s) >= 0 for s in seen) and len(set.union(*seen)) == len(seen), (j, seen)
        assert (labels[obj[rows] == -1] == -1).all()
    assert max(np.linalg.norm(rc.displacement(k, j)) for k in range(5) for j in range(1, 4)) < 2.0 - 0.25       # inside translation_frame
    args = rp.default_args(max_points=1024)

    def clouds(k, j):
        src, dst = (torch.from_numpy(raw[(t == f) & (obj == k)]).float() for f in (j, 0))
        return rp.pad_segment(src, 1024)[None], rp.pad_segment(dst, 1024)[None]

    def pose(d):
        return torch.from_numpy(rc.translation(d).reshape(1, 4, 4).copy())

    def retry(k, j, T_old):
        src, dst = clouds(k, j)
        pred = -j * rc.STEPS[k]                                               # what the two other gaps predict (they are on the line)
        T_new, aux = rp.apply_icp(args, src, dst, pose(pred), return_aux=True)
        new, old = rp.match_eval(args, src, dst, T_new), rp.match_eval(args, src, dst, T_old)
        centre = src[0, src[0, :, 3] > 0, :3].double().mean(0).numpy()
        _, report, _ = rr.select(T_new.numpy(), T_old.numpy(), int(aux["iterations"]), new[0].numpy(), new[3].numpy(), new[4].numpy(), new[5].numpy(),
                                 old[0].numpy(), centre[None], pred[None])
        return report[0]

    k, j = rc.FAULTED, rc.FAULTED_FRAME
    fixed = retry(k, j, pose(rc.displacement(k, j) + rc.FAULT))
    print("faulted pair:", fixed)
    assert np.linalg.norm(fixed[3:5] - rc.displacement(k, j)[:2]) <= rr.MAX_RESIDUAL and fixed[0] == rr.ACCEPTED and fixed[1] < fixed[2]
    k, j = rc.HONEST, rc.HONEST_FRAME
    slid = retry(k, j, pose(rc.displacement(k, j)))
    print("honest pair:", slid)
    assert slid[1] > slid[2] and slid[0] == rr.NOT_BETTER and slid[6] <= rr.MAX_RESIDUAL

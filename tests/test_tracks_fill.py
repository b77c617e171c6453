"""CPU-only: the track fill (icpflow_object_tracks_missing, icpflow_pairs_fill_candidates; csrc/tracks.hip, csrc/repair.hip;
utils_tracks, pair_judges.frame_tracks(fill=True), --tracks-fill).  The exports and their refusals (no GPU is needed for a
refusal), the flag, the numpy restatement (tests/fill_restatement.py) on hand-made tables and against np.linalg.lstsq, the
candidates' rule on thresholds hit exactly, the append, and the end-to-end scene under the oracle's clustering alone."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as fc                       # noqa: E402
import fill_restatement as fr                 # noqa: E402

F = np.float32
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
S = fc.S


@pytest.fixture(autouse=True)
def feature():
    """every test below speaks about a library that has the fill: without its exports none of them passes"""
    from icp_flow_amd import _lib, pair_judges
    assert all(hasattr(_lib._L, name) for name in ("icpflow_object_tracks_missing", "icpflow_pairs_fill_candidates"))
    assert "fill" in pair_judges.frame_tracks.__code__.co_varnames


def _lib_and_fakes():
    from icp_flow_amd import _lib
    return _lib, _lib._L, ctypes.c_void_p(4096)


# --------------------------------------------------------------------------------------------------------------------------- ABI

def test_the_exports_exist_the_constants_match_and_the_version_stays():
    from icp_flow_amd import _lib, build, utils_tracks
    assert "repair.hip" in build.SOURCES and "tracks.hip" in build.SOURCES and len(build.SOURCES) == 33          # no new source file
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "icpflow_hip.h")).read()
    for name in ("icpflow_object_tracks_missing", "icpflow_pairs_fill_candidates"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(_lib._L, name)
    assert "8(n)  track fill" in hdr and _lib.VERSION == 215 and "#define ICPFLOW_VERSION 215" in hdr
    for define, value in (("ICPFLOW_TRACK_MISSING_COLS", 14), ("ICPFLOW_TRACK_MISSING_COUNTS", 4), ("ICPFLOW_TRACK_MISSING_MAX_SLOTS", 64),
                          ("ICPFLOW_FILL_CHOICE_COLS", 8), ("ICPFLOW_FILL_COUNTS", 4)):
        assert f"#define {define} {value}\n" in hdr
    assert (_lib.TRACK_MISSING_COLS, _lib.TRACK_MISSING_COUNTS, _lib.TRACK_MISSING_MAX_SLOTS) == (fr.MISSING_COLS, fr.MISSING_COUNTS, fr.MAX_SLOTS)
    assert (_lib.FILL_CHOICE_COLS, _lib.FILL_COUNTS, _lib.FILL_MAX_ROWS) == (fr.CHOICE_COLS, fr.FILL_COUNTS, 1 << 16)
    assert utils_tracks.FILL_RADIUS == fr.FILL_RADIUS == 1.0
    assert utils_tracks.FILL_REASONS == utils_tracks.REPAIR_REASONS + ("no_candidate", "lost") and len(utils_tracks.FILL_REASONS) == 9
    assert utils_tracks.FILL_REASONS[utils_tracks.FILL_NO_CANDIDATE] == "no_candidate" and utils_tracks.FILL_REASONS[utils_tracks.FILL_LOST] == "lost"


def test_the_plan_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackParams.defaults()

    def call(**over):
        a = dict(obs=one, M=5, T=3, segments=one, num=one, G=3, Lmax=64, gap=[1, 2, 3], seconds=[0.1, 0.2, 0.3], params=good, plan=one, counts=one)
        a.update(over)
        gap = None if a["gap"] is None else (ctypes.c_int32 * len(a["gap"]))(*a["gap"])
        sec = None if a["seconds"] is None else (ctypes.c_double * len(a["seconds"]))(*a["seconds"])
        rc_ = L.icpflow_object_tracks_missing(a["obs"], a["M"], a["T"], a["segments"], a["num"], a["G"], a["Lmax"], gap, sec,
                                              ctypes.byref(a["params"]) if a["params"] is not None else None, a["plan"], a["counts"], None)
        return rc_, L.icpflow_last_error().decode()

    short = _lib.TrackParams.defaults()
    short.struct_size = 8
    cases = [(dict(M=-1), E_ARG, "negative"), (dict(T=-1), E_ARG, "negative"), (dict(G=0), E_ARG, "G must lie"), (dict(G=65, gap=list(range(65)), seconds=[0.1] * 65), E_ARG, "G must lie"),
             (dict(Lmax=0), E_ARG, "Lmax must be"), (dict(M=(1 << 16) + 1), E_LIMIT, "at most"), (dict(T=(1 << 24) + 1), E_LIMIT, "at most"),
             (dict(Lmax=4097), E_LIMIT, "at most"), (dict(params=None), E_ARG, "null pointer"), (dict(params=short), E_ARG, "struct_size"),
             (dict(gap=[1, 2, 1]), E_ARG, "distinct"), (dict(gap=[1, 2, 64]), E_ARG, "[0, 63]"), (dict(gap=[-1, 2, 3]), E_ARG, "[0, 63]"),
             (dict(seconds=[0.1, 0.0, 0.3]), E_ARG, "seconds"), (dict(seconds=[0.1, -0.2, 0.3]), E_ARG, "seconds"),
             (dict(seconds=[0.1, float("nan"), 0.3]), E_ARG, "seconds"), (dict(seconds=[0.1, 0.2, float("inf")]), E_ARG, "seconds")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("obs", "segments", "num", "gap", "seconds", "plan", "counts")]
    cases += [(dict(params=_lib.TrackParams.defaults(max_residual=bad)), E_ARG, "max_residual") for bad in (-0.5, float("nan"), float("inf"))]
    for over, code, text in cases:
        got, msg = call(**over)
        assert got == code and text in msg and msg.startswith("icpflow_object_tracks_missing"), (over, got, msg)


def test_the_candidates_refuse_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()

    def call(**over):
        a = dict(q=one, K=3, boxes=one, num=one, Lmax=64, pairs=one, P=4, stride=10, radius=1.0, max_rows=10000, choice=one, counts=one)
        a.update(over)
        rc_ = L.icpflow_pairs_fill_candidates(a["q"], a["K"], a["boxes"], a["num"], a["Lmax"], a["pairs"], a["P"], a["stride"], a["radius"], a["max_rows"],
                                              a["choice"], a["counts"], None)
        return rc_, L.icpflow_last_error().decode()

    cases = [(dict(K=-1), E_ARG, "negative"), (dict(P=-1), E_ARG, "negative"), (dict(K=(1 << 16) + 1), E_LIMIT, "at most"), (dict(Lmax=0), E_ARG, "Lmax must be"),
             (dict(Lmax=4097), E_LIMIT, "at most"), (dict(stride=0), E_ARG, "pair_stride"), (dict(max_rows=0), E_ARG, "max_rows"), (dict(pairs=None), E_ARG, "no pair rows")]
    cases += [(dict(radius=bad), E_ARG, "radius") for bad in (0.0, -1.0, float("nan"), float("inf"), float(np.nextafter(1e3, 2e3)))]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("q", "boxes", "num", "choice", "counts")]
    for over, code, text in cases:
        got, msg = call(**over)
        assert got == code and text in msg and msg.startswith("icpflow_pairs_fill_candidates"), (over, got, msg)


# ---------------------------------------------------------------------------------------------------------------- the flag

def test_the_flag_goes_with_tracks_and_the_defaults_stay():
    from icp_flow_amd import frame_pairs
    ns = frame_pairs.argument_parser().parse_args(["dir"])
    assert ns.tracks_fill is False and ns.tracks_repair is False
    assert frame_pairs.argument_parser().parse_args(["dir", "--tracks", "--tracks-fill"]).tracks_fill is True
    with pytest.raises(SystemExit, match="--tracks-fill goes with --tracks"):
        frame_pairs.main(["dir", "--tracks-fill"])
    with pytest.raises(SystemExit, match="--tracks-fill goes with --tracks"):
        frame_pairs.main(["dir", "--tracks-fill", "--tracks-log"])
    with pytest.raises(SystemExit, match="--tracks-fill is not built into --tracks-log"):
        frame_pairs.main(["dir", "--tracks", "--tracks-fill", "--tracks-log"])
    with pytest.raises(SystemExit, match="--tracks is not built into --protocol reference"):
        frame_pairs.main(["dir", "--tracks", "--tracks-fill", "--protocol", "reference"])
    assert "tracks_fill" not in frame_pairs.DEFAULT_ARGS and not hasattr(frame_pairs.default_args(), "tracks_fill")
    assert frame_pairs.DEFAULT_ARGS["max_points"] == 10000 and frame_pairs.DEFAULT_ARGS["thres_error"] == 0.2
    a = frame_pairs.default_args()
    a.tracks_fill = True
    with pytest.raises(ValueError, match="args.tracks_fill goes with args.tracks"):
        frame_pairs.run_stream(a, [], "cpu")
    a.tracks = True
    with pytest.raises(ValueError, match="args.tracks under more than one rank"):
        frame_pairs.run_stream(a, [], "cpu", rank=0, world=2)


def test_the_fill_report_sums_into_a_summary():
    import torch
    from icp_flow_amd import utils_tracks
    tracks = lambda observed, judged: SimpleNamespace(fit_counts=np.array([6, observed, judged, 3, 4]))     # noqa: E731
    done = utils_tracks.Fill(tracks(5, 4), [9, 4, 3, 3], [dict(gap=1, segment=2)], [1, 0, 0, 0, 1, 0, 0, 1, 0], ms=2.5)
    assert done.summary(tracks(5, 5)) == dict(missing=3, retried=2, accepted=1, observed_before=5, observed_after=5, judged_before=4, judged_after=5,
                                              reasons=dict(accepted=1, reject_test=0, error=0, off_prediction=0, not_better=1, abandoned=0, too_long=0,
                                                           no_candidate=1, lost=0))
    assert done.ms == 2.5 and done.retried == [dict(gap=1, segment=2)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.missing_device(torch.zeros((2, 13), dtype=torch.float64), 1, torch.zeros((1, 4, 6), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), [1], [0.1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.fill_candidates_device(torch.zeros((2, 3), dtype=torch.float64), torch.zeros((4, 16), dtype=torch.float64), torch.zeros(1, dtype=torch.int32), None)


# --------------------------------------------------------------------------------------------------------------------- the plan

def _plan(rows, gaps=(1, 2, 3), T=1, max_residual=fr.MAX_RESIDUAL, segments=None):
    seg, num, h_gap, h_sec = fc.slots(gaps, segments)
    return fr.missing(rows, T, seg, num, h_gap, h_sec, max_residual)


def test_gaps_1_2_3_seen_in_1_and_3_name_gap_2_exactly():
    plan, written, counts = _plan(fc.on_a_line(seen=(1, 3)))
    assert plan[:, 1, 0].tolist() == [0, 1, 0] and counts.tolist() == [[1, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0]]
    row = plan[1, 1]
    assert row[1:6].tolist() == [0, 5, 0, 2, 2] and row[13] == 40
    assert row[6:9].tolist() == [0.5, -0.25, 0.0625] and row[9:12].tolist() == [7.5, -3.75, 0.9375] and row[12] == 0.0
    assert plan[0, 1, 3:6].tolist() == [1, 1, 1] and not plan[0, 1, [0, 6, 7, 8, 9, 10, 11, 12]].any()         # observed in gap 1: never missing
    assert written.tolist() == [[True, True, False, False]] * 3 and (plan[~written] == fr.POISON).all()
    assert plan[:, 0, 1].tolist() == [-1, -1, -1] and not plan[:, 0, 3:13].any()                                  # the noise segment has no id


def test_seen_in_one_gap_only_is_not_eligible_and_two_rows_in_one_gap_are_one_distinct_gap():
    plan, _, counts = _plan(fc.on_a_line(seen=(1,)))
    assert counts.tolist() == [[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0]] and plan[1, 1, 3:6].tolist() == [0, 1, 1] and not plan[:, 1, 0].any()
    twice = fc.on_a_line(seen=(1,)) + fc.on_a_line(seen=(1,))
    plan, _, counts = _plan(twice)
    assert plan[1, 1, 3:6].tolist() == [0, 2, 1] and counts[1].tolist() == [1, 1, 0, 0] and not plan[1, 1, [0, 6, 7, 8, 9, 10, 11, 12]].any()
    far = fc.on_a_line(seen=(1, 3)) + [fc.obs(0, 64, 0.5, (9.0, 9.0, 9.0)), fc.obs(0, -1, 0.5, (9.0, 9.0, 9.0))]
    assert _plan(far)[0][1, 1, 4:6].tolist() == [4, 2]                                    # gaps outside [0, 63] are rows but set no bit
    plan, _, counts = _plan([fc.obs(np.nan, 1, S, (1, 1, 1))], segments=[[fc.segment(5.0, 40, np.nan)], [fc.segment(5.0, 40, 1)], [fc.segment(5.0, 40, -1)]])
    assert counts.tolist() == [[0, 0, 0, 0]] * 3                                          # a NaN id, an id >= T, no id


def test_an_observed_segment_is_never_missing():
    rows = fc.on_a_line(seen=(1, 2, 3))
    plan, _, counts = _plan(rows)
    assert not plan[:, :2, 0].any() and counts.tolist() == [[1, 0, 0, 0]] * 3 and plan[:, 1, 3].tolist() == [1, 1, 1] and plan[:, 1, 4].tolist() == [2, 2, 2]
    # observed twice in its own gap, the other gaps on their line: still not missing
    plan, _, counts = _plan(fc.on_a_line(seen=(1, 2, 2, 3)), gaps=(2,))
    assert plan[0, 1, 3:6].tolist() == [2, 2, 2] and plan[0, 1, 0] == 0.0 and counts.tolist() == [[1, 0, 0, 0]]


def test_inner_exactly_m2_is_still_missing_and_the_next_double_is_not():
    # the others: s = 0.5 each, d = (0, +-y): v = 0, inner = y^2
    rows = lambda y: [fc.obs(0, 1, 0.5, (0.0, y, 0.0)), fc.obs(0, 3, 0.5, (0.0, -y, 0.0))]   # noqa: E731
    plan, _, counts = _plan(rows(0.25), max_residual=0.25)
    assert plan[1, 1, 12] == 0.25 and plan[1, 1, 0] == 1.0 and counts[1].tolist() == [1, 1, 1, 1]
    plan, _, counts = _plan(rows(float(np.nextafter(0.25, 1.0))), max_residual=0.25)
    assert plan[1, 1, 0] == 0.0 and counts[1].tolist() == [1, 1, 1, 0] and plan[1, 1, 12] > 0.25 and plan[1, 1, 6:9].tolist() == [0, 0, 0]
    # one gap off its line by 1 m: the others do not agree, nothing is predicted from them
    plan, _, _ = _plan(fc.on_a_line(seen=(1, 3), off={3: (0.0, 1.0, 0.0)}))
    assert plan[1, 1, 0] == 0.0 and plan[1, 1, 12] > 0.2


def test_the_velocity_equals_least_squares_through_the_origin():
    """p = s_g v with v = (sum s d) / (sum s s) over the K other rows: as tests/test_tracks.py derives for the fit,
    |v - v_exact| <= (2 K + 3) u sum|s d| / sum s s to first order, u = 2^-53, and 16 u |d| / |s| is allowed for np.linalg.lstsq's own
    error; the product s_g v adds one rounding, u |s_g v|."""
    rng = np.random.default_rng(8)
    u = 2.0 ** -53
    for K in (2, 3, 8):
        for _ in range(20):
            s = 0.1 * np.arange(1, K + 1)
            d = s[:, None] * rng.normal(0, 5, 3) + rng.normal(0, 0.02, (K, 3))
            rows = [fc.obs(0, g + 1, s[g], d[g], rng.normal(0, 10, 3)) for g in range(K)]
            sg = 0.1 * (K + 1)
            seg, num, h_gap, _ = fc.slots((K + 1,))
            plan, _, counts = fr.missing(rows, 1, seg, num, h_gap, [sg], max_residual=10.0)
            assert counts.tolist() == [[1, 1, 1, 1]]
            want = np.linalg.lstsq(s[:, None], d, rcond=None)[0][0]
            for a in range(3):
                bound = (2 * K + 3) * u * np.abs(s * d[:, a]).sum() / (s ** 2).sum() + 16 * u * np.linalg.norm(d[:, a]) / np.linalg.norm(s)
                assert abs(plan[0, 1, 6 + a] - sg * want[a]) <= sg * bound + u * abs(sg * want[a]), (K, a)


def test_q_is_the_mean_landing_point_less_p_exactly_on_binary_fractions():
    rows = [fc.obs(0, 1, S, (0.25, -0.125, 0.0), (3.0, 1.5, 0.5)), fc.obs(0, 3, 3 * S, (0.75, -0.375, 0.0), (2.0, 2.25, 1.0)),
            fc.obs(0, 5, 5 * S, (1.25, -0.625, 0.0), (1.5, 1.0, 1.5)), fc.obs(0, 7, 7 * S, (1.75, -0.875, 0.0), (0.5, 3.0, 1.0))]
    seg, num, h_gap, h_sec = fc.slots((2,))
    plan, _, _ = fr.missing(rows, 1, seg, num, h_gap, h_sec)
    land = np.array([[3.25, 1.375, 0.5], [2.75, 1.875, 1.0], [2.75, 0.375, 1.5], [2.25, 2.125, 1.0]])
    p = np.array([0.5, -0.25, 0.0])
    assert plan[0, 1, 0] == 1.0 and plan[0, 1, 6:9].tolist() == p.tolist() and plan[0, 1, 9:12].tolist() == (land.mean(axis=0) - p).tolist()
    assert plan[0, 1, 9:12].tolist() == [2.25, 1.6875, 1.0]


def test_the_seeded_plans_reach_every_kind_of_row():
    seen, slots_, unwritten, negative = np.zeros(4, np.int64), 0, 0, 0
    for case in fc.random_plans(120):
        plan, written, counts = fr.missing(case["obs"], case["T"], case["segments"], case["num"], case["gaps"], case["seconds"])
        assert (counts[:, 0] >= counts[:, 1]).all() and (counts[:, 1] >= counts[:, 2]).all() and (counts[:, 2] >= counts[:, 3]).all()
        assert counts[:, 3].sum() == (plan[:, :, 0][written] == 1.0).sum() and written.sum() == np.clip(case["num"], 0, None).sum()
        seen += counts.sum(axis=0)
        slots_, unwritten, negative = slots_ + len(case["num"]), unwritten + int((~written).sum()), negative + int((case["num"] < 0).sum())
    assert (seen > 0).all() and seen[0] > seen[1] > seen[2] > seen[3] and unwritten > 0 and negative > 0


# -------------------------------------------------------------------------------------------------------------- the candidates

def test_d2_exactly_the_radius_squared_is_within_reach_and_the_next_double_is_not():
    boxes = fc.box_table([fc.box(4.0, (3.0, 4.0, 1.0))])
    choice, counts = fr.candidates([[0.0, 0.0, 0.0]], boxes, 1, [], radius=5.0)
    assert choice[0].tolist() == [0, 0, 4.0, 50, 5.0, 3.0, 4.0, 1.0] and counts.tolist() == [1, 0, 0, 1]
    choice, counts = fr.candidates([[0.0, 0.0, 9.0]], boxes, 1, [], radius=float(np.nextafter(5.0, 0.0)))
    assert choice[0].tolist() == [1, -1, 0, 0, 0, 0, 0, 0] and counts.tolist() == [0, 1, 0, 1]
    boxes = fc.box_table([fc.box(4.0, (float(np.nextafter(3.0, 4.0)), 4.0, 1.0))])
    assert fr.candidates([[0.0, 0.0, 0.0]], boxes, 1, [], radius=5.0)[0][0, 0] == 1.0
    assert fr.candidates([[0.0, 0.0, 0.0]], boxes, 0, [], radius=5.0)[1].tolist() == [0, 1, 0, 0]             # a table of no segment
    assert fr.candidates(np.zeros((0, 3)), boxes, 1, [])[1].tolist() == [0, 0, 0, 0]                          # K = 0: four zeros


def test_ties_go_to_the_lower_segment_and_to_the_lower_row():
    boxes = fc.box_table([fc.box(1.0, (0.5, 0.0, 0.0)), fc.box(2.0, (-0.5, 0.0, 0.0)), fc.box(3.0, (0.0, 0.5, 0.0)), fc.box(7.0, (10.0, 10.0, 0.0))])
    choice, counts = fr.candidates([[0.0, 0.0, 0.0]], boxes, 4, [])
    assert choice[0, :2].tolist() == [0, 0] and counts.tolist() == [1, 0, 0, 4]
    # three rows aimed at segment 3: rows 1 and 2 are equally near and nearer than row 0 -- row 1 keeps it, the others lose it
    q = [[10.25, 10.0, 0.0], [10.0, 10.125, 0.0], [10.0, 9.875, 5.0], [0.5, 0.25, 0.0]]
    choice, counts = fr.candidates(q, boxes, 4, [])
    assert choice[:, 0].tolist() == [2, 0, 2, 0] and choice[:3, 1].tolist() == [3, 3, 3] and counts.tolist() == [2, 0, 2, 4]
    assert choice[0, 2:].tolist() == [7.0, 50, 0.25, 10.0, 10.0, 0.0]                     # a loser names the segment it lost, whole
    assert choice[3, 1] == 0 and choice[3, 4] == 0.25


def test_a_matched_label_a_too_long_segment_and_a_segment_without_a_box_are_no_candidates():
    boxes = fc.box_table([fc.box(1.0, (0.0, 0.0, 0.0)), fc.box(2.0, (0.1, 0.0, 0.0), rows=10001), fc.box(3.0, (0.2, 0.0, 0.0), k=-1),
                          fc.box(4.0, (0.3, 0.0, 0.0), rows=10000), fc.box(5.0, (0.9, 0.0, 0.0))])
    choice, counts = fr.candidates([[0.0, 0.0, 0.0]], boxes, 5, [1.0, 9.0])
    assert choice[0, :3].tolist() == [0, 3, 4.0] and counts.tolist() == [1, 0, 0, 2]
    assert fr.is_candidate(boxes, 5, [1.0, 9.0], 10000).tolist() == [False, False, False, True, True]
    assert fr.candidates([[0.0, 0.0, 0.0]], boxes, 3, [1.0])[0][0].tolist() == [1, -1, 0, 0, 0, 0, 0, 0]       # rows from the number on are not read
    assert fr.candidates([[0.0, 0.0, 0.0]], boxes, 5, [1.0, 4.0, 5.0], max_rows=20000)[0][0, :2].tolist() == [0, 1]


def test_signed_zero_labels_are_one_label_and_a_nan_never_matches():
    boxes = fc.box_table([fc.box(-0.0, (0.0, 0.0, 0.0)), fc.box(np.nan, (0.5, 0.0, 0.0))])
    assert fr.is_candidate(boxes, 2, [0.0], 100).tolist() == [False, True] and fr.is_candidate(boxes, 2, [-0.0, np.nan], 100).tolist() == [False, True]
    boxes[0, 0] = 0.0
    assert fr.is_candidate(boxes, 2, [-0.0], 100).tolist() == [False, True] and fr.is_candidate(boxes, 2, [1.0], 100).tolist() == [True, True]
    # a label that float32 rounds onto a matched one is matched: the comparison is the narrowed label's
    boxes[0, 0] = 16777217.0
    assert fr.is_candidate(boxes, 2, [16777216.0], 100).tolist() == [False, True]


def test_a_nan_centre_is_out_of_reach():
    boxes = fc.box_table([fc.box(1.0, (np.nan, 0.0, 0.0)), fc.box(2.0, (0.0, np.nan, 0.0)), fc.box(3.0, (0.75, 0.0, np.nan))])
    choice, counts = fr.candidates([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], boxes, 3, [])
    assert choice[0, :2].tolist() == [0, 2] and np.isnan(choice[0, 7]) and choice[1].tolist() == [1, -1, 0, 0, 0, 0, 0, 0] and counts.tolist() == [1, 1, 0, 3]


def test_the_seeded_candidates_reach_every_reason():
    seen = np.zeros(4, np.int64)
    for seed, (K, num, P) in enumerate(((5, 40, 10), (9, 300, 100), (3, 0, 0), (20, 70, 0), (1, 1, 1))):
        case = fc.random_candidates(K, num, P, seed)
        choice, counts = fr.candidates(case["q"], case["boxes"], case["num"], case["pairs"][:, 0])
        assert counts[:3].sum() == K and counts[3] <= num
        seen += counts
    assert (seen > 0).all()


# --------------------------------------------------------------------------------------------------------------- the bookkeeping

def test_the_append_touches_no_old_row():
    rng = np.random.default_rng(2)
    pairs = np.concatenate([np.array([[3, 5], [4, 6], [7, 8]], F), rng.random((3, 8)).astype(F)], axis=1)
    T = rng.normal(size=(3, 4, 4)).astype(F)
    metrics = {k: np.array([[10.0 + c, 20.0 + c], [30.0 + c, 40.0 + c], [50.0 + c, 60.0 + c]], F) for c, k in enumerate(("errors", "inliers", "ratios", "ious"))}
    T_new = rng.normal(size=(3, 4, 4)).astype(F)
    got_pairs, got_T = fr.append(pairs, T, [[9, 1], [11, 2], [12, 3]], metrics, T_new, [True, False, True])
    assert got_pairs[:3].tobytes() == pairs.tobytes() and got_T[:3].tobytes() == T.tobytes() and got_pairs.shape == (5, 10) and got_T.shape == (5, 4, 4)
    assert got_pairs[3].tolist() == [9, 1, 10, 20, 11, 21, 12, 22, 13, 23] and got_pairs[4].tolist() == [12, 3, 50, 60, 51, 61, 52, 62, 53, 63]
    assert got_T[3].tobytes() == T_new[0].tobytes() and got_T[4].tobytes() == T_new[2].tobytes()
    none_pairs, none_T = fr.append(pairs, T, [[9, 1]], {k: v[:1] for k, v in metrics.items()}, T_new[:1], [False])
    assert none_pairs.tobytes() == pairs.tobytes() and none_T.tobytes() == T.tobytes()
    first_pairs, first_T = fr.append(np.zeros((0, 10), F), np.zeros((0, 4, 4), F), [[9, 1]], {k: v[:1] for k, v in metrics.items()}, T_new[:1], [True])
    assert first_pairs.shape == (1, 10) and first_T.tobytes() == T_new[0].tobytes()


# --------------------------------------------------------------------------------------------------------------------- the scene

def test_the_scene_is_what_the_end_to_end_test_claims_under_the_oracle():
    """Under the oracle's CPU DBSCAN alone and the synthetic truth for the registrations (every pair's transform the true
    translation, every box centre the mean of its cluster's bounding box): with object FILLED's pair deleted in gap FILLED_FRAME
    the restated plan names exactly that (gap, segment), and the restated choice is the deleted pair's source segment -- the
    prediction lies centimetres from it, the next box tens of metres away."""
    from oracle import cluster as oc
    sc = fc.scene()
    raw, t, obj = sc["arrays"]["raw_points"].astype(np.float64), sc["arrays"]["time_indice"], sc["object"]
    a = SimpleNamespace(epsilon=fc.CLUSTER["epsilon"], min_cluster_size=fc.CLUSTER["min_cluster_size"], num_clusters=fc.CLUSTER["num_clusters"])
    n0 = int((t == 0).sum())
    K = len(rc_steps())
    obs, segments, nums, boxes, pairs = [], [], [], {}, {}
    for j in range(1, fc.FRAMES):
        rows = np.concatenate([np.flatnonzero(t == 0), np.flatnonzero(t == j)])          # dst first, as cluster_frame_pair stacks them
        labels = oc.cluster_pcd(a, raw[rows], np.ones(len(rows), bool))
        ld, ls = labels[:n0], labels[n0:]
        od, os_ = obj[rows][:n0], obj[rows][n0:]
        lab_d = [int(np.unique(ld[od == k])[0]) for k in range(K)]
        lab_s = [int(np.unique(ls[os_ == k])[0]) for k in range(K)]
        assert all(len(np.unique(ld[od == k])) == 1 for k in range(K)) and len(set(lab_d)) == K and min(lab_d) >= 0
        centre = lambda pts: (pts.min(axis=0) + pts.max(axis=0)) * 0.5   # noqa: E731
        src = raw[rows][n0:]
        # the destination's segments in ascending label order, track k = object k (the same rows in every gap)
        order = np.argsort(lab_d)
        seg = np.zeros((8, 6))
        seg[:K] = [fc.segment(float(lab_d[k]), int((od == k).sum()), k) for k in order]
        segments.append(seg), nums.append(K)
        order_s = np.argsort(lab_s)
        boxes[j] = fc.box_table([fc.box(float(lab_s[k]), centre(src[os_ == k]), rows=int((os_ == k).sum())) for k in order_s], 8), [int(k) for k in order_s]
        pairs[j] = []
        for k in range(K):
            if (k, j) == (fc.FILLED, fc.FILLED_FRAME):
                continue                                                                  # the deleted pair
            pairs[j].append(float(lab_s[k]))
            obs.append(fc.obs(k, j, j * fc.SWEEP_SECONDS, fc.displacement(k, j), centre(src[os_ == k])))
    gaps = list(range(1, fc.FRAMES))
    plan, written, counts = fr.missing(obs, K, np.array(segments), nums, gaps, [g * fc.SWEEP_SECONDS for g in gaps])
    named = [(g, c) for g in range(len(gaps)) for c in range(8) if written[g, c] and plan[g, c, 0] == 1.0]
    assert len(named) == 1 and counts[:, 3].tolist() == [0, 1, 0]
    g, c = named[0]
    assert gaps[g] == fc.FILLED_FRAME and plan[g, c, 1] == fc.FILLED
    assert np.linalg.norm(plan[g, c, 6:8] - fc.displacement(fc.FILLED, fc.FILLED_FRAME)[:2]) < 0.02
    table, order_s = boxes[fc.FILLED_FRAME]
    choice, ccounts = fr.candidates(plan[g, c, 9:12][None], table, K, pairs[fc.FILLED_FRAME])
    print("plan row", plan[g, c], "choice", choice[0])
    assert ccounts.tolist() == [1, 0, 0, 1] and order_s[int(choice[0, 1])] == fc.FILLED and choice[0, 4] < 0.1
    # the box that truly leaves its line, its pair deleted where it left: the prediction lies 1 m from its box centre, at the radius itself
    assert np.linalg.norm(fc.rc.HONEST_OFFSET) == fr.FILL_RADIUS


def rc_steps():
    return fc.rc.STEPS

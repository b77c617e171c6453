"""The hand-built rows of tests/eval_rows_cases.py are what their names claim, the two numpy restatements give the reference's own
verdict on them (tests/golden/g13_seqeval_rows.npz, tools/gen_golden_seqeval.py: compute_epe_test, crop_data and calculate_metrics
run ON the thresholds), and the host half of calculate_metrics turns that table into the reference's meters.  CPU only."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_rows_cases as ec          # noqa: E402
import segment_restatement as sg      # noqa: E402
import seqeval_restatement as sr      # noqa: E402
from conftest import load_golden      # noqa: E402

FIXTURE = "g13_seqeval_rows"
REL = {"below": np.less, "at": np.equal, "above": np.greater}


def _er(p):
    with np.errstate(all="ignore"):
        return sr.errors(p.gt, p.pred)


def _numpy_flags(e, r):
    with np.errstate(all="ignore"):
        return np.stack([(e < 0.05) | (r < 0.05), (e < 0.1) | (r < 0.1), (e > 0.3) | (r > 0.1), (e > 0.3) & (r > 0.3)], axis=1)


def test_the_exact_quotients_and_roots_the_rows_rest_on():
    assert 0.25 / 5.0 == 0.05 and 0.25 / 2.5 == 0.1 and 0.75 / 2.5 == 0.3 and ec.Z_MIN == 0.3
    for v in list(ec.steps(0.05)) + list(ec.steps(0.1)) + list(ec.steps(0.3)) + [float(x) for x in ec.steps(0.25, np.float32)] + [1e-30]:
        v = np.float64(np.float32(v)) if v == 1e-30 else np.float64(v)
        assert np.sqrt(v * v) == v and np.linalg.norm(np.array([[0.0, v, 0.0]]), axis=-1)[0] == v
        assert v / (v + 1e-20) == 1.0 or v < 1e-20
    for thr in ec.THRESHOLDS:
        lo, at, hi = ec.steps(thr)
        assert lo < at < hi and at == thr and np.nextafter(lo, np.inf) == at and np.nextafter(hi, -np.inf) == at


def test_predicate_rows_are_what_they_claim():
    """e or r stands ==, < or > its threshold as the row's name says; the flags written down by hand are numpy's; the comparison that
    decides does so alone (the other quantity's half of an `or` is false and of the `and` true on all three rows of the triple)."""
    p = ec.predicate_rows()
    e, r = _er(p)
    assert np.array_equal(_numpy_flags(e, r), p.flags)
    other_half = {0: lambda e, r, q: (r if q == "e" else e) < 0.05, 1: lambda e, r, q: (r if q == "e" else e) < 0.1,
                  2: lambda e, r, q: (r > 0.1) if q == "e" else (e > 0.3), 3: lambda e, r, q: (r > 0.3) if q == "e" else (e > 0.3)}
    seen = set()
    for i in range(len(p.gt)):
        if not p.side[i]:
            continue
        v = e[i] if p.quantity[i] == "e" else r[i]
        assert REL[p.side[i]](v, p.thr[i]), p.name[i]
        assert abs(v - p.thr[i]) <= 2 * np.spacing(np.float32(p.thr[i]) if p.quantity[i] == "r" else p.thr[i]), p.name[i]   # one step: of a float32 pred for r
        for k in p.decides[i]:
            assert bool(other_half[k](e[i], r[i], p.quantity[i])) == (k == 3), (p.name[i], k)
        seen.add((p.group[i], p.thr[i], p.side[i]))
    # at the threshold every strict comparison is false; one step inside it is true
    for i in np.flatnonzero(p.side == "at"):
        for k in p.decides[i]:
            assert not p.flags[i, k], p.name[i]
    for group, thr, inside, k in (("e_alone", 0.05, "below", 0), ("e_alone", 0.1, "below", 1), ("e_alone", 0.3, "above", 3), ("e_outlier", 0.3, "above", 2),
                                  ("r_strict", 0.05, "below", 0), ("r_relax", 0.1, "below", 1), ("r_relax", 0.1, "above", 2), ("r_routlier", 0.3, "above", 3)):
        sel = (p.group == group) & (p.thr == thr)
        assert (group, thr, "at") in seen and p.flags[sel & (p.side == inside), k].all() and (sel & (p.side == inside)).sum() == 3
        assert not p.flags[sel & (p.side != inside), k].any()
    # every hand row stands in each of the three columns
    for i in np.flatnonzero(p.group != "order")[::3]:
        assert np.array_equal(np.roll(p.gt[i], 1), p.gt[i + 1], equal_nan=True) and np.array_equal(np.roll(p.pred[i], 2), p.pred[i + 2], equal_nan=True)
    # zero truth and the rows that are not finite
    zero = p.group == "zero_truth"
    assert (r[zero][:3] == 0).all() and np.allclose(r[zero][3:], 1e-10, rtol=1e-6) and (e[zero][3:] == np.float64(np.float32(1e-30))).all()
    by = lambda s: np.flatnonzero(np.char.startswith(p.name, s))   # noqa: E731
    assert np.isnan(e[by("pred NaN")]).all() and np.isnan(e[by("gt NaN")]).all()
    assert np.isinf(e[by("pred +inf")]).all() and np.isinf(r[by("pred +inf")]).all()
    assert np.isinf(e[by("gt +inf")]).all() and np.isnan(r[by("gt +inf")]).all()
    assert (~p.finite).sum() == 12 and (p.group[~p.finite] == "not_finite").all()


def test_operation_order_rows_straddle_in_exact_rationals():
    """At least five rows per threshold whose e, rounded operation by operation as numpy does, and whose e by either contracted form
    (one rounding per fma, evaluated in exact rationals) fall on different sides of the threshold; the rational evaluation is itself
    checked against numpy on the separately rounded form."""
    rows = ec.order_rows()
    rn = lambda q: Fraction(float(q))   # noqa: E731
    for thr in ec.THRESHOLDS:
        mine = [d for t, d in rows if t == thr]
        assert len(mine) >= 5
        for d in mine:
            x, y, z = (Fraction(v) for v in d)
            separate = math.sqrt(float(rn(rn(rn(x * x) + rn(y * y)) + rn(z * z))))
            assert separate == ec.e_separate(d) == float(np.linalg.norm(np.array([d]), axis=-1)[0])
            fused = math.sqrt(float(rn(z * z + rn(y * y + rn(x * x)))))
            assert fused == ec.e_fused(d, "y")
            want = ec.verdict(separate, thr)
            assert ec.verdict(fused, thr) != want and ec.verdict(ec.e_fused(d, "x"), thr) != want
            assert abs(separate - thr) <= 2 * np.spacing(thr) and abs(fused - thr) <= 2 * np.spacing(thr)
    p = ec.predicate_rows()
    assert (p.group == "order").sum() == len(rows) and (p.pred[p.group == "order"] == 0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_crop_rows_are_what_they_claim(dtype):
    """Coordinates == the bound (as numpy compares an array of that type) or one step off; the kept flags written down by hand are
    numpy's, the reference's crop_data's, and what the kernel's fp64 test gives with the thresholds _threshold_for hands it."""
    from icp_flow_amd import utils_eval
    c, g = ec.crop_rows(dtype), load_golden(FIXTURE)
    tag = "f64" if dtype is np.float64 else "f32"
    assert np.array_equal(g[f"crop_{tag}_pts"], c.pts, equal_nan=True) and g[f"crop_{tag}_pts"].dtype == dtype
    assert np.array_equal(g[f"crop_{tag}_keep"], c.keep_xyz) and np.array_equal(g[f"crop_{tag}_keep_xy"], c.keep_xy)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(sr.keep_mask(ec.args_for(3), c.pts), c.keep_xyz)
        assert sr.keep_mask(ec.args_for(3, eval_ground=True), c.pts).all()
        rx, ry, zmin = (utils_eval._threshold_for(v, c.pts) for v in (ec.RANGE_X, ec.RANGE_Y, ec.Z_MIN))
        assert (rx, ry, zmin) == tuple(float(dtype(v)) for v in (ec.RANGE_X, ec.RANGE_Y, ec.Z_MIN))
        wide = c.pts.astype(np.float64)
        xy = (np.abs(wide[:, 0]) < rx) & (np.abs(wide[:, 1]) < ry)
        assert np.array_equal(xy, c.keep_xy) and np.array_equal(xy & (wide[:, 2] > zmin), c.keep_xyz)
        assert sg.z_threshold(ec.Z_MIN, c.pts) == zmin                   # the segment table's crop reads the same threshold
    for axis, bound in ((0, dtype(ec.RANGE_X)), (1, dtype(ec.RANGE_Y))):
        for sign in "+-":
            v = {side: c.pts[list(c.name).index(f"{'xy'[axis]} {sign}{side}"), axis] for side in ec.SIDES}
            assert abs(v["at"]) == bound and abs(v["below"]) == np.nextafter(bound, dtype(0)) and abs(v["above"]) == np.nextafter(bound, dtype(np.inf))
            assert np.sign(v["at"]) == (1 if sign == "+" else -1)
    z = {side: c.pts[list(c.name).index(f"z {side}"), 2] for side in ec.SIDES}
    assert z["at"] == dtype(ec.Z_MIN) and z["below"] == np.nextafter(z["at"], dtype(-1)) and z["above"] == np.nextafter(z["at"], dtype(1))
    if dtype is np.float32:
        # a float32 point AT float32(32.3) fails the crop, although the same number is < 32.3 in fp64 ...
        i = list(c.name).index("x +at")
        assert float(c.pts[i, 0]) < ec.RANGE_X and not c.keep_xyz[i]
    else:
        # ... and as a float64 point it passes
        i = list(c.name).index("x float32(32.3)")
        assert c.pts[i, 0] == float(np.float32(ec.RANGE_X)) and c.keep_xyz[i] and c.keep_xyz[list(c.name).index("z float32(0.3)")]


def test_the_restatements_give_the_reference_flags_on_the_thresholds():
    """Row by row: the reference's compute_epe_test on one row (its e, its four flags) against both restatements' e, r and
    predicates -- equal bit for bit in e, equal in every flag, NaN where it has NaN."""
    g, p = load_golden(FIXTURE), ec.predicate_rows()
    assert np.array_equal(g["pred_gt"], p.gt, equal_nan=True) and np.array_equal(g["pred_pred"], p.pred, equal_nan=True)
    assert list(g["pred_name"]) == list(p.name) and g["pred_gt"].dtype == np.float64 and g["pred_pred"].dtype == np.float32
    assert np.array_equal(g["pred_flags"].astype(bool), p.flags)
    with np.errstate(all="ignore"):
        for e, r in (sr.errors(p.gt, p.pred), sg.errors(p.gt, p.pred)):
            assert np.array_equal(e, g["pred_e"], equal_nan=True)
            assert np.array_equal(sg.predicates(e, r).T, p.flags) and np.array_equal(_numpy_flags(e, r), p.flags)


@pytest.mark.parametrize("eg", [0, 1], ids=["crop", "eval_ground"])
@pytest.mark.parametrize("tag", ["64", "32"])
def test_meters_from_the_numpy_table_equal_the_reference(tag, eg):
    """seqeval_restatement.table_numpy on the F = 3 arrangement of the predicate and crop rows, through update_meters: every meter
    as the reference's calculate_metrics left it -- counts exact, fractions equal as float32, NaN where the reference has NaN."""
    from icp_flow_amd import utils_eval
    g, prefix = load_golden(FIXTURE), f"m{tag}__"
    data, pred, F = ec.fixture_sample(g, prefix)
    s = ec.meter_sample(np.float64 if tag == "64" else np.float32)
    assert all(np.array_equal(data[k], s.data[k], equal_nan=True) and data[k].dtype == s.data[k].dtype for k in data)
    assert np.array_equal(pred, s.pred, equal_nan=True)
    with np.errstate(all="ignore"):
        table, esum, kept0 = sr.table_numpy(ec.args_for(F, eg), data, pred)
    meters = utils_eval.update_meters(ec.args_for(F, eg), utils_eval.new_metric_table(F), table, esum, kept0)
    nans = ec.check_meters(meters, g, eg, prefix, table)
    assert nans > 0 and np.isnan(meters["dynamic_fg_2"].epe_avg) and not np.isnan(meters["static_2"].epe_avg)
    assert not np.isnan(meters["overall_1"].epe_avg) and float(meters["overall_1"].num) == table[1, 0, 0]
    # the crop faces decide the weights: kept rows of frame 0 are the crop rows' hand flags plus the predicate sample's three
    c = ec.crop_rows(np.float64 if tag == "64" else np.float32)
    assert kept0 == (len(c.pts) if eg else int(c.keep_xyz.sum())) + 3


def test_the_segment_restatement_counts_by_hand():
    pts, lab, gt, pred, z_min, hand = ec.segment_cloud()
    with np.errstate(all="ignore"):
        table, e, _, _ = sg.table_numpy(pts, lab, pred, gt, z_min)
    assert len(table) == 14 and list(table[:, 0]) == sorted(hand)
    for row in table:
        rows, kept, *counts = hand[row[0]]
        assert (row[1], row[2]) == (rows, kept) and list(row[4:8]) == counts, row[0]
    assert np.isnan(table[12, 3]) and (table[13, 2:14] == 0).all() and table[13, 1] == 6
    assert (pts[lab == ec.ON_Z_MIN_ID, 2] == z_min).all() and not np.isfinite(e[lab == ec.NOT_FINITE_ID]).all()
    pts, lab, gt, pred, z_min, hand = ec.open_crop_cloud()
    table = sg.table_numpy(pts, lab, pred, gt, None)[0]
    assert z_min == -np.inf and [(r[1], r[2]) for r in table] == [hand[4.0], hand[7.0]]


def test_tiles_chunks_and_seams_are_where_they_are_said_to_be():
    s = ec.metric_samples()
    a = s["all_gaps_in_a_tile"]
    t, sd, fb = a.data["time_indice"], a.data["sd_labels"], a.data["fb_labels"]
    first = [int(np.flatnonzero(t[:64] == j)[0]) for j in range(1, 16)]
    assert a.F == 16 and first == sorted(first, reverse=True) and set(t[:64]) == set(range(1, 16))
    assert all({(int(x), int(y)) for x, y in zip(sd[t == j], fb[t == j])} >= {(x, y) for x in range(3) for y in range(3)} for j in range(1, 16))
    t = s["tile_without_a_gap"].data["time_indice"]
    assert not ((t[64:128] >= 1) & (t[64:128] < 4)).any() and ((t[:64] >= 1) & (t[:64] < 4)).all() and len(t) == 256
    t = s["lane_0_and_lane_63"].data["time_indice"]
    rows = np.flatnonzero(t)
    assert sorted(t[rows[rows % 64 == 0]]) == list(range(1, 16)) and sorted(t[rows[rows % 64 == 63]]) == list(range(1, 16)) and len(rows) == 30
    assert len(s["m_65"].pred) == 65 and len(s["m_0_F_1"].pred) == 0 and s["m_0_F_16"].F == 16 and s["F_1"].F == 1
    w = s["two_workgroups_and_a_tail"]
    m = len(w.pred)
    assert m == 2 * 2048 + 65 and w.where == [0, 63, 64, 2047, 2048, m - 1]
    p = ec.predicate_rows()
    on_edge = {tuple(r) for r in p.gt[(p.side == "at") | (p.group == "order")]}
    assert all(tuple(w.data["scene_flow"][r]) in on_edge for r in w.where)
    lab = ec.seam_labels()
    sizes = np.bincount(lab.astype(np.int64))
    chunks = -(-sizes // ec.CHUNK)
    assert len(sizes) == 1030 and 13000 < len(lab) < 17000
    assert list(chunks[1020:1028]) == [2, 2, 3, 1, 3, 2, 2, 2] and (chunks[:1020] == 1).all() and (chunks[1028:] == 1).all()
    assert {1024, 1025, 2048, 2049} <= set(sizes[1020:1028]) and chunks[1023] > 0     # the last segment of the plan's first round carries into the second
    assert not (np.diff(lab) >= 0).all()                                            # rows interleaved


def test_float32_truth_is_judged_differently_on_exactly_these_rows():
    """The kernel's contract: scene_flow widened, judged in fp64.  The reference judges a float32 scene_flow in float32: it
    subtracts, takes the norm and compares there (the thresholds rounded to float32).  On the rows below -- and on no other of the
    predicate rows -- its flags differ from the fp64 judgement of the same rounded truth (COVERAGE.md, named deviations)."""
    g, p = load_golden(FIXTURE), ec.predicate_rows()
    gt32 = p.gt.astype(np.float32)
    with np.errstate(all="ignore"):
        e32 = np.linalg.norm(gt32 - p.pred, axis=-1)
        r32 = e32 / (np.linalg.norm(gt32, axis=-1) + 1e-20)
        assert e32.dtype == np.float32 and np.array_equal(e32, g["pred32_e"], equal_nan=True)
        assert np.array_equal(_numpy_flags(e32, r32), g["pred32_flags"].astype(bool))
        wide = _numpy_flags(*sr.errors(gt32, p.pred))                   # what the kernel computes of a float32 truth
    differ = (wide != g["pred32_flags"].astype(bool)).any(axis=1)
    print("float32 truth: rows judged differently:", list(p.name[differ]))
    # float32(0.3) = 0.300000012 lies ABOVE the double 0.3 (float32(0.05) and float32(0.1) lie above theirs too, but `<` is false on
    # both sides of them): all nine rows whose truth rounds to float32(0.3) have e > 0.3 in fp64 and e == float32(0.3) in float32, in
    # Routlier (e alone) and in Outlier (small r); r one float32 step above 0.3 rounds onto float32(0.3) in the float32 division.
    hand = {("e_alone", 0.3), ("e_outlier", 0.3)}
    want = np.array([(p.group[i], p.thr[i]) in hand or (p.group[i], p.side[i]) == ("r_routlier", "above") for i in range(len(p.gt))])
    assert np.array_equal(differ[p.group != "order"], want[p.group != "order"]) and want.sum() == 21
    # an operation-order row's truth rounded to float32 is another row, 1e-9 off its threshold; float32 rounds its e onto or across
    # float32(thr) on these seven (positions in the group), recorded from the reference's verdict in the fixture
    assert list(np.flatnonzero(differ[p.group == "order"])) == [0, 6, 7, 8, 10, 13, 14]
    # with a float64 truth -- what every other fixture stores -- there is nothing to differ: the reference computes in fp64 too
    assert g["pred_e"].dtype == np.float64


@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_time_indices_and_labels_are_compared_before_they_are_narrowed(kind):
    """narrow_time_indices: a value keeps its frame only if it EQUALS an integer of [0, F) on its own type, as the reference's
    `time_indice == j` decides; 2^32 + 1 is not gap 1 and 1.5 is not gap 1."""
    from icp_flow_amd import utils_eval
    F = 3
    for name, values, inside in ec.time_index_cases(F):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(inside, np.any([values == j for j in range(F)], axis=0)), name
        got = utils_eval.narrow_time_indices(values if kind == "numpy" else torch.from_numpy(values), F)
        got = got if kind == "numpy" else got.numpy()
        assert got.dtype == np.int32 and ((got >= 0) & (got < F) == inside).all(), name
        with np.errstate(invalid="ignore"):
            assert (got[inside] == values[inside]).all() and (got[~inside] == -1).all(), name
    for name, values, want in ec.label_cases():
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.where(values == 0, 0, np.where(values == 1, 1, 2)), want), name

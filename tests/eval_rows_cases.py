"""Hand-built rows for the evaluation's row rules (csrc/rowerr.hpp: row_error / row_predicates / crop_keep), shared by
tools/gen_golden_seqeval.py (which records the reference's own verdict on them in g13_seqeval_rows.npz), tests/test_eval_rows_cases.py
(every row is what its name claims) and tests/test_gpu_eval_rows.py (the four kernels).  numpy only.  Not a test module.

Every expected flag below is written down by construction, never computed from e and r:
  * sqrt(x * x) is |x| in binary floating point, so a row with one non-zero difference has e = |that difference| exactly;
  * 0.25 / 5, 0.25 / 2.5 and 0.75 / 2.5 are the doubles 0.05, 0.1 and 0.3 (one correctly rounded division of exact operands
    whose real quotient is the decimal the literal is rounded from)."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

F32 = np.float32
THRESHOLDS = (0.05, 0.1, 0.3)
SIDES = ("below", "at", "above")
RANGE_X = RANGE_Y = 32.3
RANGE_Z, GROUND_SLACK = 0.0, 0.3
Z_MIN = RANGE_Z + GROUND_SLACK                        # 0.3 exactly
NAN, INF = float("nan"), float("inf")
CHUNK = 1024                                          # rows of a chunk, segments of a plan round (csrc/segeval.hip)
ORDER_ROWS_PER_THRESHOLD = 5
ORDER_SEED, ORDER_CANDIDATES, ORDER_WALK = 20261021, 4000, 6


def steps(v, dtype=np.float64):
    """-> (one step below, at, one step above) v in `dtype`"""
    v = dtype(v)
    return np.nextafter(v, dtype(-np.inf)), v, np.nextafter(v, dtype(np.inf))


def args_for(F, eval_ground=False):
    return SimpleNamespace(num_frames=int(F), eval_ground=bool(eval_ground), range_x=RANGE_X, range_y=RANGE_Y, range_z=RANGE_Z,
                           ground_slack=GROUND_SLACK)


# ---- the operation-order rows ---------------------------------------------------------------------------------------------
def e_separate(d):
    """numpy's norm: sqrt((x*x + y*y) + z*z), each operation rounded by itself"""
    x, y, z = (np.float64(v) for v in d)
    return float(np.sqrt((x * x + y * y) + z * z))


def e_fused(d, inner_first="y"):
    """the contracted form in exact rationals: sqrt(fma(z, z, fma(y, y, x*x))), or with inner_first "x" fma(z, z, fma(x, x, y*y));
    float(Fraction) is the correctly rounded double, math.sqrt the correctly rounded root"""
    x, y, z = (Fraction(float(v)) for v in d)
    a, b = (x, y) if inner_first == "y" else (y, x)
    inner = Fraction(float(b * b + Fraction(float(a * a))))
    return math.sqrt(float(z * z + inner))


def verdict(e, thr):
    """the comparison the reference makes of e with this threshold: e < 0.05, e < 0.1, e > 0.3"""
    return e > thr if thr == 0.3 else e < thr


@lru_cache(maxsize=None)
def order_rows():
    """Seeded search: a random direction scaled to the threshold, z walked a few doubles either way; kept when the separately
    rounded e and BOTH fused forms give different verdicts at the threshold.  -> tuple of (thr, (x, y, z))"""
    rng = np.random.default_rng(ORDER_SEED)
    found = []
    for thr in THRESHOLDS:
        have = 0
        for _ in range(ORDER_CANDIDATES):
            u = rng.normal(size=3)
            g = u / np.linalg.norm(u) * thr
            for k in range(-ORDER_WALK, ORDER_WALK + 1):
                z = g[2]
                for _ in range(abs(k)):
                    z = np.nextafter(z, np.inf if k > 0 else -np.inf)
                d = (float(g[0]), float(g[1]), float(z))
                want = verdict(e_separate(d), thr)
                if verdict(e_fused(d, "y"), thr) != want and verdict(e_fused(d, "x"), thr) != want:
                    found.append((thr, d))
                    have += 1
                    break
            if have == ORDER_ROWS_PER_THRESHOLD:
                break
        assert have == ORDER_ROWS_PER_THRESHOLD, (thr, have)
    return tuple(found)


# ---- the predicate rows -----------------------------------------------------------------------------------------------
def _flags_e(thr, side, e_true):
    """the four flags of a row whose r is 1 and whose e stands `side` of thr; e_true: the verdict of e at thr"""
    return {0.05: (e_true, True, True, False), 0.1: (False, e_true, True, False), 0.3: (False, False, True, e_true)}[thr]


@lru_cache(maxsize=None)
def predicate_rows():
    """-> SimpleNamespace(name [n], gt float64 [n,3], pred float32 [n,3], flags bool [n,4] (strict, relax, outlier, Routlier),
    group [n], quantity [n] ('e', 'r' or ''), thr [n], side [n] ('below' / 'at' / 'above' / ''), decides [n] (tuple of predicate
    columns the quantity decides alone), finite [n]).  Every row but the operation-order ones three times: its components rolled
    by 0, 1 and 2 columns."""
    rows = []

    def add(group, name, gt, pred, flags, quantity="", thr=0.0, side="", decides=(), roll=True):
        for k in range(3 if roll else 1):
            rows.append((f"{name}/roll{k}", group, tuple(np.roll(np.float64(gt), k)), tuple(np.roll(F32(pred), k)), tuple(flags), quantity,
                         thr, side, tuple(decides)))

    for thr in THRESHOLDS:                                  # e alone, r = g / (g + 1e-20) = 1
        for side, g in zip(SIDES, steps(thr)):
            lt, gt_ = side == "below", side == "above"
            add("e_alone", f"e {side} {thr}", (g, 0, 0), (0, 0, 0), _flags_e(thr, side, gt_ if thr == 0.3 else lt), "e", thr, side,
                {0.05: (0,), 0.1: (1,), 0.3: (3,)}[thr])
    for side, g in zip(SIDES, steps(0.3)):                  # e = g, r about 0.0375: strict and relax hold by r, Outlier by e alone
        add("e_outlier", f"e {side} 0.3, small r", (g, 8, 0), (0, 8, 0), (True, True, side == "above", False), "e", 0.3, side, (2,))
    for side, p in zip(SIDES, steps(0.25, F32)):            # e = p = 0.25, r = p / 5
        add("r_strict", f"r {side} 0.05", (5, 0, 0), (5, 0, p), (side == "below", True, False, False), "r", 0.05, side, (0,))
    for side, p in zip(SIDES, steps(0.25, F32)):            # e = p = 0.25, r = p / 2.5
        add("r_relax", f"r {side} 0.1", (2.5, 0, 0), (2.5, 0, p), (False, side == "below", side == "above", False), "r", 0.1, side, (1, 2))
    for side, p in zip(SIDES, steps(0.75, F32)):            # e = p = 0.75, r = p / 2.5
        add("r_routlier", f"r {side} 0.3", (2.5, 0, 0), (2.5, 0, p), (False, False, True, side == "above"), "r", 0.3, side, (3,))
    add("zero_truth", "gt 0, pred 0", (0, 0, 0), (0, 0, 0), (True, True, False, False))             # r = 0 / 1e-20 = 0
    add("zero_truth", "gt 0, pred 1e-30", (0, 0, 0), (1e-30, 0, 0), (True, True, False, False))     # e = 1e-30, r = 1e-10
    # not finite.  e NaN: every comparison false.  pred +inf: e = inf, r = inf / |gt| = inf: both outlier flags.  gt +inf: e = inf,
    # r = inf / inf = NaN: Outlier by e, Routlier false.
    add("not_finite", "pred NaN", (1, 0, 0), (NAN, 0, 0), (False, False, False, False))
    add("not_finite", "pred +inf", (1, 0, 0), (INF, 0, 0), (False, False, True, True))
    add("not_finite", "gt NaN", (NAN, 1, 0), (0, 1, 0), (False, False, False, False))
    add("not_finite", "gt +inf", (INF, 1, 0), (0, 1, 0), (False, False, True, False))
    for thr, d in order_rows():                             # pred 0: e = |gt| as numpy rounds it, r = 1
        v = verdict(e_separate(d), thr)
        add("order", f"order {thr} {d[2].hex()}", d, (0, 0, 0), _flags_e(thr, "", v), "e", thr, "", (), roll=False)
    cols = list(zip(*rows))
    gt, pred = np.array(cols[2], np.float64), np.array(cols[3], F32)
    return SimpleNamespace(name=np.array(cols[0]), group=np.array(cols[1]), gt=gt, pred=pred, flags=np.array(cols[4], bool),
                           quantity=np.array(cols[5]), thr=np.array(cols[6]), side=np.array(cols[7]), decides=cols[8],
                           finite=np.isfinite(gt).all(axis=1) & np.isfinite(pred).all(axis=1))


# ---- the crop rows ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def crop_rows(dtype, bound=RANGE_X):
    """Points of type `dtype` on the faces of the crop |x| < bound, |y| < bound, z > 0.3 (bound 32.3; 32.0 for the suites whose
    helpers fix it), the bound being the one numpy compares such an array with: dtype(32.3), dtype(0.3).
    -> SimpleNamespace(name, pts dtype [n,3], keep_xyz, keep_xy bool [n])"""
    dtype = np.dtype(dtype).type
    rows = []

    def add(name, p, xyz, xy):
        rows.append((name, tuple(dtype(v) for v in p), bool(xyz), bool(xy)))

    add("inside", (1, -2, 1), True, True)
    add("far outside", (100, 0, 1), False, False)
    for axis in (0, 1):
        for sign in (1, -1):
            for side, v in zip(SIDES, steps(bound, dtype)):
                p = [0, 0, 1]
                p[axis] = sign * v
                add(f"{'xy'[axis]} {'+' if sign > 0 else '-'}{side}", p, side == "below", side == "below")
        for v, tag in ((NAN, "NaN"), (INF, "+inf"), (-INF, "-inf")):
            p = [0, 0, 1]
            p[axis] = v
            add(f"{'xy'[axis]} {tag}", p, False, False)
    for side, v in zip(SIDES, steps(Z_MIN, dtype)):
        add(f"z {side}", (0, 0, v), side == "above", True)
    add("z NaN", (0, 0, NAN), False, True)
    add("z +inf", (0, 0, INF), True, True)
    add("z -inf", (0, 0, -INF), False, True)
    if dtype is np.float64 and float(F32(bound)) != bound:
        # the float32 bounds as float64 points: float32(32.3) = 32.29999923706055 < 32.3 passes, float32(0.3) = 0.30000001192092896 > 0.3 passes
        add("x float32(32.3)", (float(F32(bound)), 0, 1), True, True)
        add("y -float32(32.3)", (0, -float(F32(bound)), 1), True, True)
        add("z float32(0.3)", (0, 0, float(F32(Z_MIN))), True, True)
    cols = list(zip(*rows))
    return SimpleNamespace(name=np.array(cols[0]), pts=np.array(cols[1], dtype), keep_xyz=np.array(cols[2]), keep_xy=np.array(cols[3]))


def nine_labels(i):
    """row i -> (sd, fb): the nine pairs over {0, 1, 2} in turn (2: neither 0 nor 1)"""
    i = np.asarray(i)
    return i % 3, (i // 3) % 3


def crop_sample(dtype, bound=RANGE_X):
    """Every crop row three times, as frame 0, 1 and 2 of an F = 3 sample; e = (i % 8) / 8 exactly (gt = (e, 0, 0), pred = 0), so
    every sum is exact in any order.  -> (data, pred, classes float64 [m])"""
    c = crop_rows(dtype, bound)
    n = len(c.pts)
    pts, tim = np.tile(c.pts, (3, 1)), np.repeat(np.arange(3), n)
    i = np.arange(3 * n)
    sd, fb = nine_labels(i)
    gt = np.zeros((3 * n, 3))
    gt[:, 0] = (i % 8) / 8.0
    data = dict(raw_points=pts, time_indice=tim.astype(np.int64), sd_labels=sd.astype(np.int64), fb_labels=fb.astype(np.int64), scene_flow=gt)
    return data, np.zeros((3 * n, 3), F32), (i % 5).astype(np.float64)


# ---- gaps, classes, sizes: samples for icpflow_seq_metrics -----------------------------------------------------------------------
def _sample(F, tim, gt=None, pred=None, sd=None, fb=None, pts=None, exact=False):
    m = len(tim)
    i = np.arange(m)
    if gt is None:                                     # e = (i % 16) / 16 exactly: on both sides of every e threshold, sums exact
        gt = np.zeros((m, 3))
        gt[:, 1] = (i % 16) / 16.0
        pred, exact = np.zeros((m, 3), F32), True
    nsd, nfb = nine_labels(i)
    data = dict(raw_points=np.tile(np.array([[1.0, 1.0, 1.0]]), (m, 1)) if pts is None else pts, time_indice=np.asarray(tim, np.int64),
                sd_labels=(nsd if sd is None else np.asarray(sd)).astype(np.int64),
                fb_labels=(nfb if fb is None else np.asarray(fb)).astype(np.int64), scene_flow=np.asarray(gt, np.float64))
    return SimpleNamespace(F=int(F), data=data, pred=np.asarray(pred, F32), exact=exact)


def predicate_sample():
    """F = 3.  The finite predicate rows alternate between gap 1 (all nine label pairs) and gap 2 (sd 0 or neither); the
    not-finite rows are gap 2, sd = fb = 1: they touch overall_2, dynamic_2, dynamic_fg_2, the same classes of row 0, nothing else."""
    p = predicate_rows()
    n = len(p.gt)
    i = np.arange(n)
    tim = np.where(p.finite, 1 + i % 2, 2)
    sd, fb = nine_labels(i // 2)
    sd = np.where(tim == 2, np.where(sd == 1, 2, sd), sd)
    sd, fb = np.where(p.finite, sd, 1), np.where(p.finite, fb, 1)
    # a few rows of frame 0 in front (main.py:218: their flow is zero)
    z = np.zeros((3, 3))
    return _sample(3, np.concatenate([[0, 0, 0], tim]), np.concatenate([z, p.gt]), np.concatenate([z.astype(F32), p.pred]),
                   np.concatenate([[0, 0, 0], sd]), np.concatenate([[0, 0, 0], fb]))


def meter_sample(dtype):
    """What the fixture records the reference's calculate_metrics on: predicate_sample followed by crop_sample(dtype), the
    predicate rows at the point (1, 1, 1) in the points' type."""
    s = predicate_sample()
    data, pred, _ = crop_sample(dtype)
    out = {k: np.concatenate([s.data[k].astype(data[k].dtype), data[k]]) for k in data}
    return SimpleNamespace(F=3, data=out, pred=np.concatenate([s.pred, pred]), exact=False)


def metric_samples():
    """-> {name: sample} of the shapes where seq_metrics_kernel's gap loop, tiles and grid can go wrong"""
    out = {"predicates": predicate_sample()}
    # a tile of 64 rows holding all fifteen gaps in descending order of first row, then every (sd, fb) pair in every gap
    head = np.concatenate([15 - np.arange(15), 1 + (np.arange(49) * 7) % 15])
    tail = np.repeat(np.arange(1, 16), 9)
    s = _sample(16, np.concatenate([head, tail]))
    s.data["sd_labels"][64:], s.data["fb_labels"][64:] = np.tile(np.arange(9) % 3, 15), np.tile(np.arange(9) // 3, 15)
    out["all_gaps_in_a_tile"] = s
    # a tile whose rows are all frame 0 or outside [0, F), between two ordinary tiles
    dead = np.resize(np.array([0, -1, 4, 100, -2 ** 31, 0, 2 ** 31 - 1]), 64)
    out["tile_without_a_gap"] = _sample(4, np.concatenate([1 + np.arange(64) % 3, dead, 1 + np.arange(64) % 3, dead]))
    # one row per gap at lane 0 and at lane 63, every other lane frame 0
    tim = np.zeros(30 * 64, np.int64)
    tim[np.arange(15) * 64] = np.arange(1, 16)
    tim[(15 + np.arange(15)) * 64 + 63] = np.arange(1, 16)
    out["lane_0_and_lane_63"] = _sample(16, tim)
    # the last tile is one row, and that row stands on a threshold
    p = predicate_rows()
    at = np.flatnonzero((p.side == "at") | (p.group == "order"))
    s = _sample(3, 1 + np.arange(65) % 2)
    s.data["scene_flow"][64], s.pred[64], s.exact = p.gt[at[0]], p.pred[at[0]], False
    out["m_65"] = s
    # two workgroups and a tail: the threshold rows at the first and last lane of a tile, of a workgroup, of the sample
    m = 2 * 2048 + 65
    s = _sample(3, 1 + np.arange(m) % 2)
    where = [0, 63, 64, 2047, 2048, m - 1]
    for k, row in enumerate(where):
        for q, src in enumerate(at[k::len(where)]):     # several threshold rows per place: neighbours of it, still at its tile's edge
            r = row + q if row in (0, 64, 2048) else row - q
            s.data["scene_flow"][r], s.pred[r] = p.gt[src], p.pred[src]
    s.exact, s.where = False, where
    out["two_workgroups_and_a_tail"] = s
    out["F_1"] = _sample(1, np.resize(np.array([0, 0, 1, -1, 0]), 130))
    out["m_0_F_1"], out["m_0_F_16"] = _sample(1, np.zeros(0, np.int64)), _sample(16, np.zeros(0, np.int64))
    return out


# ---- segments: clouds for icpflow_seq_segment_table --------------------------------------------------------------------------
SEGMENT_IDS = (-1e8, -1.0, 0.0, 1.0, 2.0, 3.0, 5.0, 8.0, 13.0, 21.0, 34.0, 55.0)   # the dozen the finite predicate rows are dealt over
NOT_FINITE_ID, ON_Z_MIN_ID = 89.0, 144.0


def segment_cloud():
    """-> (pts float64, labels float32, gt, pred, z_min, hand): finite predicate row i in segment SEGMENT_IDS[i % 12] at z = 1, the
    not-finite rows a segment of their own, six rows with z == z_min a segment of their own.  hand: {label: (rows, kept, 4 counts)}"""
    p = predicate_rows()
    fin, bad = np.flatnonzero(p.finite), np.flatnonzero(~p.finite)
    lab = np.concatenate([np.array(SEGMENT_IDS)[np.arange(len(fin)) % 12], np.full(len(bad), NOT_FINITE_ID), np.full(6, ON_Z_MIN_ID)])
    rows = np.concatenate([fin, bad, fin[:6]])
    pts = np.tile(np.array([[1.0, -2.0, 1.0]]), (len(rows), 1))
    pts[-6:, 2] = Z_MIN
    hand = {}
    for ident in SEGMENT_IDS + (NOT_FINITE_ID,):
        sel = rows[lab == ident]
        hand[ident] = (len(sel), len(sel)) + tuple(int(p.flags[sel, k].sum()) for k in range(4))
    hand[ON_Z_MIN_ID] = (6, 0, 0, 0, 0, 0)
    return pts, lab.astype(F32), p.gt[rows], p.pred[rows], Z_MIN, hand


def open_crop_cloud():
    """z_min = -inf: rows with z = -inf or NaN are dropped, everything else -- +inf, -1e300, -0.0 -- is kept.  Two segments."""
    z = np.array([-INF, NAN, INF, -1e300, -0.0, 0.0, 1.0, -INF, NAN, 2.0])
    pts = np.stack([np.arange(10.0), -np.arange(10.0), z], axis=1)
    lab = np.array([4, 4, 4, 4, 4, 7, 7, 7, 7, 7], F32)
    gt = np.zeros((10, 3))
    gt[:, 0] = np.arange(10) / 8.0
    return pts, lab, gt, np.zeros((10, 3), F32), -INF, {4.0: (5, 3), 7.0: (5, 3)}


SEAM_SEGMENTS = 1030
SEAM_SIZES = {1020: 1025, 1021: 2048, 1022: 2049, 1023: 1024, 1024: 2049, 1025: 1025, 1026: 2048, 1027: 1536}


def seam_labels():
    """1030 segments (labels 0 .. 1029), the plan's round being 1024 segments: segments 1020 .. 1027 have one, two and three
    chunks on both sides of it, the others one row each.  Rows interleaved by a fixed permutation.  -> labels float32"""
    sizes = [SEAM_SIZES.get(k, 1) for k in range(SEAM_SEGMENTS)]
    lab = np.repeat(np.arange(SEAM_SEGMENTS, dtype=F32), sizes)
    return lab[np.random.default_rng(1030).permutation(len(lab))]


# ---- the fixture's meters ------------------------------------------------------------------------------------------------
METRICS = ("epe", "accs", "accr", "outlier", "Routlier")
CLASSES = ("overall", "static", "static_bg", "static_fg", "dynamic", "dynamic_fg")
U = 2.0 ** -53


def fixture_sample(g, prefix):
    """-> (data, pred, F) of a meter_sample stored in g13_seqeval_rows.npz"""
    data = {k: g[prefix + k] for k in ("raw_points", "time_indice", "sd_labels", "fb_labels", "scene_flow")}
    return data, g[prefix + "pred_flow"], int(g[prefix + "num_frames"])


def check_meters(meters, g, eg, prefix, counts):
    """Every meter against what the reference's calculate_metrics left in g13_seqeval_rows.npz: the number of updates, num and
    the weights exactly; fractions equal as float32; NaN where the reference has NaN and inf where it has inf; a finite mean
    error within 2 n 2^-53 of the reference's (two summation orders of the cell's n values, tests/test_gpu_seqeval.py).
    counts: the table's counts [F,6,6]."""
    names = [str(n) for n in g[prefix + "meter_names"]]
    assert list(meters) == names
    F = int(g[prefix + "num_frames"])
    same32 = lambda a, b: bool(np.float32(a) == np.float32(b)) or bool(np.isnan(a) and np.isnan(b))   # noqa: E731
    nans = 0
    for i, name in enumerate(names):
        m = meters[name]
        cls, row = name.rsplit("_", 1)
        n = max(float(counts[int(row) if 1 <= int(row) < F else 0, CLASSES.index(cls), 0]), 1.0)
        nd = int(g[prefix + f"eg{eg}_ndata"][i])
        assert len(m.epe_data) == nd and len(m.num_data) == nd, name
        assert float(m.num) == float(g[prefix + f"eg{eg}_num"][i]), name
        want_avg = g[prefix + f"eg{eg}_avg"][i]
        if not nd:
            assert all(float(getattr(m, k + "_avg")) == 0.0 for k in METRICS), name
            continue
        assert float(m.num_data[0]) == float(g[prefix + f"eg{eg}_num_data"][i]), name
        want = g[prefix + f"eg{eg}_data"][i]
        for k, metric in enumerate(METRICS):
            for a, b in ((getattr(m, metric + "_data")[0], want[k]), (getattr(m, metric + "_avg"), want_avg[k])):
                a, b = float(a), float(b)
                nans += int(np.isnan(b))
                if k and not np.isnan(b):
                    assert same32(a, b), (name, metric, a, b)
                else:
                    assert (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 2 * n * U * abs(b), (name, metric, a, b)
    return nans


# ---- time indices and labels as a sample may store them -------------------------------------------------------------------
def time_index_cases(F=3):
    """-> list of (name, array, inside bool [n]): values that equal an integer of [0, F) and values that equal none"""
    return [("int64", np.array([0, 1, 2, 2 ** 32, 2 ** 32 + 1, -2 ** 31 - 1, -1, F, 1], np.int64),
             np.array([1, 1, 1, 0, 0, 0, 0, 0, 1], bool)),
            ("float64", np.array([0.0, 1.0, 1.5, 2.0, NAN, INF, -0.5, 2.0 ** 32 + 1, 1.0], np.float64), np.array([1, 1, 0, 1, 0, 0, 0, 0, 1], bool)),
            ("float32", np.array([0.0, 1.0, 1.5, 2.0, NAN, -INF, 0.99999994, 3.0, 1.0], F32), np.array([1, 1, 0, 1, 0, 0, 0, 0, 1], bool))]


def label_cases():
    """-> list of (name, array, what the reference's `== 0` / `== 1` make of each value: 0, 1 or 2)"""
    return [("float64", np.array([0.0, 1.0, 0.5, NAN, -0.0, 1.0, 0.0, 2.0, 1.0]), np.array([0, 1, 2, 2, 0, 1, 0, 2, 1])),
            ("bool", np.array([0, 1, 1, 0, 0, 1, 0, 1, 1], bool), np.array([0, 1, 1, 0, 0, 1, 0, 1, 1])),
            ("int64", np.array([0, 1, 2 ** 32, 2 ** 32 + 1, -1, 1, 0, 2 ** 31, 1], np.int64), np.array([0, 1, 2, 2, 2, 1, 0, 2, 1]))]

"""Plain fp64 numpy restatement of the per-segment evaluation (icpflow_seq_segment_table and utils_flow.flow_evaluation), written
from the reference's source: the masks of utils_flow.py:86-95, compute_epe_test (utils_eval.py:162-180), the crop of
utils_debug.py:37-46, len / mean of utils_flow.py:110 and the translation of :123.  Shared by the CPU and the GPU tests."""
import math
import os
import re
import warnings

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
COLS = 16
CHUNK = 1024                     # C of csrc/segeval.hip: rows of a chunk
FIXTURES = ["g14_segments_f32", "g14_segments_f64"]
E_THRESHOLDS = (0.05, 0.1, 0.3)


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def errors(gt, pred):
    """e, r per row as compute_epe_test has them (utils_eval.py:163-168), fp64: numpy's norm is sqrt((x*x + y*y) + z*z)"""
    gt = np.asarray(gt, np.float64)
    d = gt - np.asarray(pred).astype(np.float64)
    e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    r = e / (np.sqrt((gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1]) + gt[:, 2] * gt[:, 2]) + 1e-20)
    return e, r


def predicates(e, r):
    """utils_eval.py:170-180 -> bool [4, n]: strict, relax, outlier, Routlier"""
    return np.stack([(e < 0.05) | (r < 0.05), (e < 0.1) | (r < 0.1), (e > 0.3) | (r > 0.1), (e > 0.3) & (r > 0.3)])


def z_threshold(z_min, points):
    """the threshold as numpy compares it with the stored coordinates (utils_debug.py:38): rounded to a float32 array's type"""
    if z_min is None:
        return -np.inf
    return float(np.float32(z_min)) if np.asarray(points).dtype == np.float32 else float(z_min)


def table_numpy(points, labels, flow_pd=None, flow_gt=None, z_min=None):
    """-> (table [S,16] with every sum an exactly rounded math.fsum, per-row e or None, sum |coordinate| [S,3],
    sum |x + f| [S,3]): what icpflow_seq_segment_table returns up to the order of its additions."""
    pts = np.asarray(points)[:, 0:3].astype(np.float64)
    labels = np.asarray(labels, np.float32)
    keep = pts[:, 2] > z_threshold(z_min, points)
    uniq = np.unique(labels)
    S = len(uniq)
    table, absx, absm = np.zeros((S, COLS)), np.zeros((S, 3)), np.zeros((S, 3))
    e = None
    if flow_gt is not None:
        e, r = errors(flow_gt, flow_pd)
        p = predicates(e, r)
        moved = pts + np.asarray(flow_pd)[:, 0:3].astype(np.float64)     # each term rounded once
    for c, lab in enumerate(uniq):
        seg = labels == lab
        k = seg & keep
        table[c, 0:3] = lab, seg.sum(), k.sum()
        for a in range(3):
            table[c, 8 + a] = math.fsum(pts[k, a])
            absx[c, a] = math.fsum(np.abs(pts[k, a]))
        if e is not None:
            table[c, 3] = math.fsum(e[k])
            table[c, 4:8] = p[:, k].sum(axis=1)
            for a in range(3):
                table[c, 11 + a] = math.fsum(moved[k, a])
                absm[c, a] = math.fsum(np.abs(moved[k, a]))
    return table, e, absx, absm


def check_table(got, want, absx, absm, flows=True):
    """counts exactly; every sum within (n - 1) 2^-53 sum |term| of the exactly rounded sum (math.fsum) -- the textbook bound of
    any summation order of n terms (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 to first order; for
    non-negative terms sum |term| is the sum itself).  One term, or none: equality."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got[:, [0, 1, 2, 4, 5, 6, 7, 14, 15]], want[:, [0, 1, 2, 4, 5, 6, 7, 14, 15]])
    n = np.maximum(want[:, 2] - 1.0, 0.0)
    assert (np.abs(got[:, 3] - want[:, 3]) <= n * U * want[:, 3]).all(), np.abs(got[:, 3] - want[:, 3]).max()
    assert (np.abs(got[:, 8:11] - want[:, 8:11]) <= n[:, None] * U * absx).all()
    assert (np.abs(got[:, 11:14] - want[:, 11:14]) <= n[:, None] * U * absm).all()
    if not flows:
        assert (got[:, [3, 4, 5, 6, 7, 11, 12, 13]] == 0).all()


def epe_test(flow_pred, flow_gt):
    """compute_epe_test (utils_eval.py:137-182) without a mask -> five numbers in its types; NaN for no row"""
    e, r = errors(flow_gt, flow_pred)
    with np.errstate(all="ignore"):
        return (e.mean(),) + tuple(q.astype(np.float32).mean() for q in predicates(e, r))


def reference_numbers(g, crop):
    """Everything tools/gen_golden_segments.py recorded for one crop setting, from the fixture's inputs, the way the
    reference computes it: segments of np.unique(labels.astype(int)) AFTER the crop (utils_debug.py:37-46 crops the labels),
    means in the points' stored dtype."""
    src, dst = g["src_points"], g["dst_points"]
    keep = src[:, 2] > float(g["z_min"]) if crop else np.ones(len(src), bool)      # (numpy rounds the scalar to float32 points' type)
    src, ls, fp, fg, sd = src[keep], g["src_labels"][keep], g["flow_pd"][keep], g["flow_gt"][keep], g["sd_label"][keep]
    ld = g["dst_labels"]
    unqs = np.unique(ls.astype(int))
    rec = {k: [] for k in ("epe", "accs", "accr", "outlier", "routlier", "len_i", "len_j", "mean_i", "mean_j", "moved", "translation")}
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (numpy's mean of no destination row: NaN, as for the reference)
        for unq in unqs:
            i, j = ls == unq, ld == unq
            xi, xj = src[i, 0:3], dst[j, 0:3]
            for name, val in zip(("epe", "accs", "accr", "outlier", "routlier"), epe_test(fp[i], fg[i])):
                rec[name].append(float(val))
            rec["len_i"].append(len(xi)); rec["len_j"].append(len(xj))
            rec["mean_i"].append(xi.mean(0).astype(np.float64)); rec["mean_j"].append(xj.mean(0).astype(np.float64))
            moved = (xi + fp[i]).mean(0)
            rec["moved"].append(moved.astype(np.float64))
            rec["translation"].append(float(np.linalg.norm(moved - xi.mean(0))))
        frame = []
        for mask in (None, sd == 0, sd == 1):
            if mask is not None and not mask.any():
                frame.append([np.nan] * 5 + [0.0])
                continue
            m = epe_test(fp if mask is None else fp[mask], fg if mask is None else fg[mask])
            frame.append([float(x) for x in m] + [float(len(fp) if mask is None else mask.sum())])
    out = {k: np.array(v) for k, v in rec.items()}
    out["labels"] = unqs.astype(np.int64)
    out["frame_rows"] = np.array(frame)
    return out


def mean_bound(n, absmean, dtype):
    """|difference| allowed between two means of the same n terms added in different orders in `dtype`'s precision: each side
    within n u mean|term| of the exact mean (n - 1 additions and the division, or the term's own rounding), u of the coarser
    side -- the reference adds float32 points in float32"""
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else U
    return 2.0 * np.maximum(n, 1) * u * absmean


def same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


def margin(g):
    """the MARGIN CONDITION of tools/gen_golden_segments.py on the stored values -> True when it holds"""
    e, r = errors(g["flow_gt"], g["flow_pd"])
    ok = all((np.abs(e - t) > 1e-9 * t).all() and (np.abs(r - t) > 1e-9 * t).all() for t in E_THRESHOLDS)
    z = g["src_points"][:, 2].astype(np.float64)
    for zmin in (float(g["z_min"]), float(np.float32(g["z_min"]))):
        ok = ok and bool((np.abs(z - zmin) > 1e-9 * abs(zmin)).all())
    for tag in ("crop_", "all_"):
        epe = g[tag + "epe"]
        ok = ok and bool((np.abs(epe[~np.isnan(epe)] - 2.0) > 2e-9).all())
    return ok


def normalise(text):
    """a printed line up to numpy's formatting of arrays: runs of blanks collapsed, none after '[' or before ']'"""
    text = re.sub(r"\s+", " ", text.strip())
    return text.replace("[ ", "[").replace(" ]", "]")


def interleaved_labels(sizes, ids, seed):
    """labels of segments of the given sizes, rows interleaved (a random permutation), float32"""
    rng = np.random.default_rng(seed)
    lab = np.concatenate([np.full(n, i, np.float32) for n, i in zip(sizes, ids)]) if len(sizes) else np.zeros(0, np.float32)
    return lab[rng.permutation(len(lab))]


def random_cloud(labels, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    m = len(labels)
    pts = rng.uniform(-40, 40, size=(m, 3))
    pts[:, 2] = rng.uniform(-0.5, 2.0, size=m)
    gt = rng.normal(size=(m, 3)) * rng.uniform(0.0, 1.5, size=(m, 1))
    pred = (gt + rng.normal(size=(m, 3)) * rng.uniform(0.0, 0.4, size=(m, 1))).astype(np.float32)
    return pts.astype(dtype), gt, pred


def check_report(rep, g, crop):
    """a SegmentReport against the fixture: shared with tests/test_gpu_segments.py"""
    tag = "crop_" if crop else "all_"
    has = rep.n > 0
    assert np.array_equal(rep.label[has].astype(np.int64), g[tag + "labels"])
    assert np.array_equal(rep.n[has], g[tag + "len_i"]) and np.array_equal(rep.len_j[has], g[tag + "len_j"])
    assert np.isnan(rep.epe[~has]).all() and np.isnan(rep.accs[~has]).all() and np.isnan(rep.mean_i[~has]).all()
    for k in ("accs", "accr", "outlier", "routlier"):
        assert getattr(rep, k).dtype == np.float32
        assert all(same_f32(a, b) for a, b in zip(getattr(rep, k)[has], g[tag + k])), k
    n = g[tag + "len_i"]
    assert (np.abs(rep.epe[has] - g[tag + "epe"]) <= mean_bound(n, g[tag + "epe"], np.float64)).all()
    dt = g["src_points"].dtype
    for got, k, cnt in ((rep.mean_i[has], "mean_i", n), (rep.mean_j[has], "mean_j", g[tag + "len_j"]), (rep.moved[has], "moved", n)):
        want = g[tag + k]
        assert np.array_equal(np.isnan(got), np.isnan(want)), k
        assert ((np.abs(got - want) <= mean_bound(cnt[:, None], 45.0, dt)) | np.isnan(want)).all(), k
    assert (np.abs(rep.translation[has] - g[tag + "translation"]) <= 6 * mean_bound(n, 45.0, dt)).all()
    pairs = g["pairs"]
    for k in np.flatnonzero(has):
        idx = np.flatnonzero(pairs[:, 0] == rep.label[k])
        if len(idx) == 1:
            assert rep.pair_index[k] == idx[0] and rep.matched_dst[k] == pairs[idx[0], 1]
            assert np.abs(rep.rotation_zyx_deg[k] - g["euler_zyx_deg"][idx[0]]).max() <= 1e-9
        else:
            assert rep.pair_index[k] == -1 and rep.matched_dst[k] == -1 and np.isnan(rep.rotation_zyx_deg[k]).all()


def check_lines(lines, g, crop):
    """the printed text against the reference's, up to numpy's formatting of arrays: the same lines in the same order, every
    word equal except inside [...] (means: float32 arrays print 8 digits, ours are float64), where the numbers agree to 1e-4
    relative -- what 8 printed digits of a float32 mean resolve"""
    tag = "crop_" if crop else "all_"
    want = [normalise(x) for x in re.split(r"\n(?=eval segment:|predictions with|matched pair:|pose:|transform:|translation:|rotation:)",
                                              str(g[tag + "segment_text"]).strip())]
    got = [normalise(x) for x in lines]
    assert len(got) == len(want), (len(got), len(want))
    number = re.compile(r"-?\d+\.?\d*(?:e[-+]?\d+)?")
    for a, b in zip(got, want):
        assert number.sub("#", a) == number.sub("#", b), (a, b)
        x, y = np.array([float(v) for v in number.findall(a)]), np.array([float(v) for v in number.findall(b)])
        assert (np.abs(x - y) <= 1e-4 * np.maximum(np.abs(y), 1.0)).all(), (a, b)
        assert a.split("[")[0] == b.split("[")[0], (a, b)     # everything before the first array: equal text
    assert sum(x.startswith("eval segment:") for x in got) >= 5 and sum(x.startswith("rotation:") for x in got) == 1

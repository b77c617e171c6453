"""A plain fp64 numpy loop over rows restating icpflow_seq_class_table (include/icpflow_hip.h), written from its description
there, and helpers over the g15 fixtures, shared by tests/test_classes.py and tests/test_gpu_classes*.py.  Not a test module."""
import math

import numpy as np

import argo_restatement as ar
import seqeval_restatement as sr

SPEED_EDGES, ERROR_EDGES = (0.5 * 0.1, 2.0 * 0.1), (0.05, 0.1)
CLASS_LO, ROWS = -1, 33
BACKGROUND_ROWS = (0, 6, 9, 10, 14, 22, 23)          # file values -1, 5, 8, 9, 13, 21, 22
U = 2.0 ** -53


def row_speed(gt):
    gt = np.asarray(gt, np.float64)
    x, y, z = gt[:, 0], gt[:, 1], gt[:, 2]
    return np.sqrt((x * x + y * y) + z * z)


class Cells:
    """counts int64 [G,S,E]; e and speed: per cell (g, s) the list of the rows' values in row order; kept0, outside"""

    def __init__(self, G, S, E):
        self.counts = np.zeros((G, S, E), np.int64)
        self.e = [[[] for _ in range(S)] for _ in range(G)]
        self.speed = [[[] for _ in range(S)] for _ in range(G)]
        self.kept0 = self.outside = 0

    def sums(self, which="e"):
        """math.fsum per cell -> float64 [G,S]"""
        lists = self.e if which == "e" else self.speed
        return np.array([[math.fsum(c) for c in row] for row in lists])

    def bounds(self, which="e"):
        """(n - 1) 2^-53 sum |x| per cell: what any order of n - 1 additions stays within of the exact sum (to first order; the
        bound tests/test_gpu_segments.py derives for a sequential sum holds for every summation tree of depth <= n - 1)"""
        lists = self.e if which == "e" else self.speed
        return np.array([[max(len(c) - 1, 0) * U * math.fsum(abs(x) for x in c) for c in row] for row in lists])

    def sequential(self, which="e"):
        lists = self.e if which == "e" else self.speed
        out = np.zeros((len(lists), len(lists[0])))
        for g, row in enumerate(lists):
            for s, c in enumerate(row):
                acc = 0.0
                for x in c:
                    acc += x
                out[g, s] = acc
        return out


def table(args, data, pred, classes, speed_edges=SPEED_EDGES, error_edges=ERROR_EDGES, class_lo=CLASS_LO, G=ROWS, keep=None):
    """-> Cells.  data: raw_points, time_indice, scene_flow (numpy); args: num_frames and calculate_metrics' crop (`keep`: a
    row mask of the caller's instead, for the crop in x and y only).  What a row is worth is computed for all rows at once
    with numpy's own operations; the table is filled by a loop over the rows in row order."""
    F = int(args.num_frames)
    raw, t = np.asarray(data["raw_points"]), np.asarray(data["time_indice"])
    keep = sr.keep_mask(args, raw) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        e, _ = sr.errors(data["scene_flow"], pred)
        speed = row_speed(data["scene_flow"])
        S, E = len(speed_edges) + 1, len(error_edges) + 1
        bucket = sum(((speed >= edge).astype(np.int64) for edge in speed_edges), np.zeros(len(t), np.int64))
        split = sum(((e >= edge).astype(np.int64) for edge in error_edges), np.zeros(len(t), np.int64))
        cls = np.asarray(classes, np.float64)
        named = np.isfinite(cls) & (cls == np.floor(cls)) & (cls >= class_lo) & (cls <= class_lo + G - 2)
        row = np.where(named, np.where(named, cls, 0.0) - class_lo, G - 1).astype(np.int64)
    out = Cells(G, S, E)
    out.outside = int(((t < 0) | (t >= F)).sum())
    out.kept0 = int((keep & (t == 0)).sum())
    counted = keep & (t >= 1) & (t < F)
    for i, g, s, k, ei, si in zip(*(a[counted].tolist() for a in (np.arange(len(t)), row, bucket, split, e, speed))):
        out.counts[g, s, k] += 1
        out.e[g][s].append(ei)
        out.speed[g][s].append(si)
    return out


def fixture_sample(name):
    """A g15 fixture as class_table reads it -> (data dict of numpy arrays with `classes`, predicted flow float32 [m,3])"""
    arrays, pred = ar.file_arrays(name)
    s = ar.sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"], arrays["pc1_flows_valid_idx"],
                  arrays["pc2_flows_valid_idx"], (5, 8, 9, 13, 21, 22))
    s["raw_points"] = s["raw_points"].astype(arrays["pc1"].dtype)       # the file's own dtype: numpy's crop comparison
    v1 = ar.index_list(arrays["pc1_flows_valid_idx"])
    m2 = len(s["time_indice"]) - len(v1)
    s["classes"] = np.concatenate([np.full(m2, np.nan), np.asarray(arrays["pc1_classes"])[v1].astype(np.float64)])
    return s, pred


def marginals(counts, esum):
    """The reference's six classes from a table of ROWS x 3 speed buckets: static = bucket 0, dynamic = the others,
    background = BACKGROUND_ROWS.  counts [G,S,E], esum [G,S] -> {class: (rows, sum of e)}; sums in ascending row order, then
    buckets"""
    n = counts.sum(axis=2)
    G = n.shape[0]
    bg = list(BACKGROUND_ROWS)
    fg = [r for r in range(G) if r not in bg]
    every = list(range(G))

    def part(rows, buckets):
        total, rows_n = 0.0, 0
        for r in rows:
            for s in buckets:
                total, rows_n = total + esum[r, s], rows_n + int(n[r, s])
        return rows_n, total

    moving = range(1, n.shape[1])
    return {"overall": part(every, range(n.shape[1])), "static": part(every, (0,)), "static_bg": part(bg, (0,)),
            "static_fg": part(fg, (0,)), "dynamic": part(every, moving), "dynamic_fg": part(fg, moving)}


def check_against_recorded(name, setting, counts, esum, rel=1e-12):
    """The marginals against what the reference recorded in the fixture: rows == <setting>_num, sum / rows within `rel`
    (relative) of <setting>_avg[:, 0].  -> the largest relative difference seen"""
    g = ar.load(name)
    names = [str(n) for n in g["meter_names"]]
    worst = 0.0
    for cls, (n, total) in marginals(counts, esum).items():
        i = names.index(cls + "_1")
        assert n == int(g[setting + "_num"][i]), (name, setting, cls, n, g[setting + "_num"][i])
        if n:
            want = float(g[setting + "_avg"][i, 0])
            diff = abs(total / n - want) / abs(want)
            worst = max(worst, diff)
            assert diff <= rel, (name, setting, cls, total / n, want)
    return worst

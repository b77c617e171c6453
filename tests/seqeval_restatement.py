"""A plain numpy restatement of what icpflow_seq_metrics and icpflow_seq_gt_flow compute (include/icpflow_hip.h), and the
g13 fixtures' access helpers, shared by tests/test_seqeval.py and tests/test_gpu_seqeval*.py.  Not a test module."""
from types import SimpleNamespace

import numpy as np

from conftest import load_golden

CLASSES = ("overall", "static", "static_bg", "static_fg", "dynamic", "dynamic_fg")
METRICS = ("epe", "accs", "accr", "outlier", "Routlier")
U = 2.0 ** -53


def crop_args(g, eval_ground, prefix=""):
    return SimpleNamespace(num_frames=int(g[prefix + "num_frames"]), eval_ground=bool(eval_ground), range_x=float(g[prefix + "range_x"]),
                           range_y=float(g[prefix + "range_y"]), range_z=float(g[prefix + "range_z"]),
                           ground_slack=float(g[prefix + "ground_slack"]))


def sample(g, prefix=""):
    """the `data` dict of the reference's calculate_metrics out of a g13 fixture"""
    return {k: g[prefix + k] for k in ("raw_points", "time_indice", "sd_labels", "fb_labels", "scene_flow")}


def errors(gt, pred):
    """e and r per row with numpy's own operations (utils_eval.py:163-168)"""
    gt, pred = np.asarray(gt, np.float64), np.asarray(pred)
    e = np.linalg.norm(gt - pred, axis=-1)
    return e, e / (np.linalg.norm(gt, axis=-1) + 1e-20)


def keep_mask(args, raw):
    """utils_eval.py:33-38 / 186-189 as calculate_metrics applies it (numpy compares in the array's own type)"""
    if args.eval_ground:
        return np.ones(len(raw), bool)
    return (np.abs(raw[:, 0]) < args.range_x) & (np.abs(raw[:, 1]) < args.range_y) & (raw[:, 2] > args.range_z + args.ground_slack)


def table_numpy(args, data, pred):
    """-> (table int64 [F,6,6] with zeros where the sums of e go, esum float64 [F,6], kept rows of frame 0)"""
    F = int(args.num_frames)
    raw, t = np.asarray(data["raw_points"]), np.asarray(data["time_indice"])
    sd, fb = np.asarray(data["sd_labels"]), np.asarray(data["fb_labels"])
    keep = keep_mask(args, raw)
    e, r = errors(data["scene_flow"], pred)
    preds = ((e < 0.05) | (r < 0.05), (e < 0.1) | (r < 0.1), (e > 0.3) | (r > 0.1), (e > 0.3) & (r > 0.3))
    masks = (np.ones(len(t), bool), sd == 0, (sd == 0) & (fb == 0), (sd == 0) & (fb == 1), sd == 1, (sd == 1) & (fb == 1))
    table, esum = np.zeros((F, 6, 6), np.int64), np.zeros((F, 6))
    for j in range(1, F):
        for c, mask in enumerate(masks):
            sel = keep & (t == j) & mask
            table[j, c, 0] = sel.sum()
            esum[j, c] = e[sel].sum()
            for k, p in enumerate(preds):
                table[j, c, 2 + k] = (sel & p).sum()
    table[0] = table[1:].sum(axis=0)
    esum[0] = esum[1:].sum(axis=0)
    return table, esum, int((keep & (t == 0)).sum())


def gt_flow_numpy(raw, t, inst, ego, tsfm):
    """dataset_pca.py:66-69 restated: ((R0 x + R1 y) + R2 z) + t per coordinate, twice, minus the raw point"""
    p = np.asarray(raw, np.float64)

    def apply(T, x):
        return np.stack([((T[:, i, 0] * x[:, 0] + T[:, i, 1] * x[:, 1]) + T[:, i, 2] * x[:, 2]) + T[:, i, 3] for i in range(3)], axis=1)

    x = apply(ego[t], p)
    x = apply(tsfm[inst, t], x)
    return x - p


def gt_flow_bound(raw, ego, tsfm):
    """64 * 2^-53 * M, M = max |p| + max |t_ego| + max |t_inst| (Euclidean norms): see test_scene_flow_against_g13"""
    M = (np.linalg.norm(np.asarray(raw, np.float64), axis=1).max() + np.linalg.norm(ego[:, :3, 3], axis=-1).max() +
         np.linalg.norm(tsfm[..., :3, 3], axis=-1).max())
    return 64.0 * U * M


def load(name):
    return load_golden(name)


def reference_table(g, eg, prefix=""):
    """The reference's counts recovered from what its meters stored: n of a cell is the weight of its per-gap update,
    a predicate's count round(fraction * n) (a float32 fraction of fewer than 2^24 points pins the integer).
    -> (table int64 [F,6,6] without the sums of e, mean e [F,6] (NaN where the reference has none), kept rows of frame 0)"""
    F = int(g[prefix + "num_frames"])
    idx = {str(n): i for i, n in enumerate(g[prefix + "meter_names"])}
    ndata, num_data, data = g[prefix + f"eg{eg}_ndata"], g[prefix + f"eg{eg}_num_data"], g[prefix + f"eg{eg}_data"]
    table, epe = np.zeros((F, 6, 6), np.int64), np.full((F, 6), np.nan)
    for c, cls in enumerate(CLASSES):
        for j in range(1, F):
            i = idx[f"{cls}_{j}"]
            if ndata[i]:
                n = int(num_data[i])
                table[j, c, 0] = n
                if n:
                    table[j, c, 2:] = np.rint(data[i, 1:].astype(np.float64) * n).astype(np.int64)
                    epe[j, c] = data[i, 0]
        n0 = int(table[1:, c, 0].sum())
        table[0, c, 0] = n0
        i = idx[f"{cls}_0"]
        if ndata[i] and n0:
            table[0, c, 2:] = np.rint(data[i, 1:].astype(np.float64) * n0).astype(np.int64)
            epe[0, c] = data[i, 0]
    kept0 = int(num_data[idx["overall_0"]]) - int(table[0, 0, 0])
    return table, epe, kept0


def same_f32(a, b):
    a, b = np.float32(a), np.float32(b)
    return bool(a == b) or bool(np.isnan(a) and np.isnan(b))


def check_meters(meters, g, eg, epe_bound, prefix=""):
    """Every meter against what the reference's calculate_metrics left in the fixture: num, the number of updates and their
    weights exactly, fractions equal as float32 (NaN where the reference has NaN), mean errors within epe_bound(value, n)."""
    names = [str(n) for n in g[prefix + "meter_names"]]
    assert list(meters) == names
    F = int(g[prefix + "num_frames"])
    counts = reference_table(g, eg, prefix)[0]
    for i, name in enumerate(names):
        m = meters[name]
        cls, row = name.rsplit("_", 1)
        n = max(float(counts[int(row) if 1 <= int(row) < F else 0, CLASSES.index(cls), 0]), 1.0)    # values summed in this cell
        nd = int(g[prefix + f"eg{eg}_ndata"][i])
        assert len(m.epe_data) == nd and len(m.num_data) == nd, name
        assert float(m.num) == float(g[prefix + f"eg{eg}_num"][i]), name
        want_avg = g[prefix + f"eg{eg}_avg"][i]
        if nd:
            assert float(m.num_data[0]) == float(g[prefix + f"eg{eg}_num_data"][i]), name
            want = g[prefix + f"eg{eg}_data"][i]
            for k, metric in enumerate(METRICS):
                got, got_avg = getattr(m, metric + "_data")[0], getattr(m, metric + "_avg")
                if k == 0:
                    for a, b in ((got, want[0]), (got_avg, want_avg[0])):
                        assert (np.isnan(a) and np.isnan(b)) or abs(float(a) - float(b)) <= epe_bound(abs(float(b)), n), (name, a, b)
                else:
                    assert same_f32(got, want[k]) and same_f32(got_avg, want_avg[k]), (name, metric, got, want[k], got_avg, want_avg[k])
        else:
            assert all(float(getattr(m, metric + "_avg")) == 0.0 for metric in METRICS), name

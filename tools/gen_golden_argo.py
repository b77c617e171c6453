#!/usr/bin/env python3
"""Generate tests/golden/g15_argo_*.npz: the REFERENCE's own Argoverse 2 loader (dataset_argo.Dataset_argo.__init__ and
load_data_pca, dataset_argo.py:15-101) and its sequence evaluation (utils_eval.calculate_metrics) on file-form samples.
Runs only where the reference is (CPU, numpy); the fixtures hold inputs and recorded results, no reference source text.
Third-party modules the reference imports and that cannot be installed are the stand-ins of tools/standins, as for
tools/gen_golden_seqeval.py.

Every sample is written as <root>/<split>_zero_flow/<log>/<name>.npz into a temporary tree, so that the reference's class
finds and loads it unmodified.  Recorded per file: what load_data_pca returns (raw_points, time_indice, sd_labels, fb_labels,
scene_flow), the object's background_idxes, and -- for a predicted flow -- every meter's num, *_avg, *_data after one
calculate_metrics call with num_frames = 2 under three settings: main.py's default ranges (32 / 32 / 0 / 0.3), main.sh:38's
(10000 / 10000 / -10000 / 0), and eval_ground.

g15_argo_demo.npz: the reference's demo.npz, one real Argoverse 2 sample.  Its valid rows ARE tests/golden/g8_demo.npz's
point_src / point_dst / gt_flow (asserted here), so points, flow and prediction (g8's `flow`) are not stored again: only the
valid rows' classes (int8) and the recorded labels and meters.
g15_argo_{f32_int,f32_float,f64}.npz: three synthetic files of 700 points per cloud -- float32 with int8 classes and sorted
index lists; float32 with float32 classes and boolean masks; all float64 with sorted index lists.  Rows that no index selects
are NaN (a class that cannot be: 99).  Every background index, -1 and several foreground ids occur, each both static and dynamic.

MARGIN CONDITIONS (asserted here, re-asserted by tests/test_argo.py from the stored values): no |flow| within 1e-6 (relative)
of 0.05; no e or r within 1e-9 (relative) of a predicate threshold.  The seed of a synthetic file is the first one, counting
up from its base, for which the reference's own numbers meet them.

Usage:  python tools/gen_golden_argo.py
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tools", "standins"))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402

import dataset_argo  # noqa: E402  (reference)
import utils_eval  # noqa: E402  (reference)

OUT = os.path.join(REPO, "tests", "golden")
CLASSES = ("overall", "static", "static_bg", "static_fg", "dynamic", "dynamic_fg")
METRICS = ("epe", "accs", "accr", "outlier", "Routlier")
SETTINGS = {"default": dict(range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3, eval_ground=False),    # main.py:69-73, 113
            "argo": dict(range_x=10000.0, range_y=10000.0, range_z=-10000.0, ground_slack=0.0, eval_ground=False),   # main.sh:38
            "ground": dict(range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3, eval_ground=True)}
SAMPLE_KEYS = ("raw_points", "time_indice", "sd_labels", "fb_labels", "scene_flow")
FOREGROUND = (0, 1, 3, 7, 17, 19, 30)          # ids that are neither -1 nor a background index
N = 700


def reference_load(arrays, name="sample"):
    """The arrays as a file in a temporary <split>_zero_flow/<log>/ tree -> (load_data_pca's dict, background_idxes)"""
    root = tempfile.mkdtemp()
    try:
        log = os.path.join(root, "val_zero_flow", "log0")
        os.makedirs(log)
        if isinstance(arrays, str):
            shutil.copy(arrays, os.path.join(log, name + ".npz"))
        else:
            np.savez(os.path.join(log, name + ".npz"), **arrays)
        with contextlib.redirect_stdout(io.StringIO()):
            ds = dataset_argo.Dataset_argo(SimpleNamespace(root=root, split="val", num_frames=2))
            assert len(ds) == 1
            data = ds.load_data_pca(ds.seq_paths[0])
        return data, np.array(ds.background_idxes, dtype=np.int64)
    finally:
        shutil.rmtree(root)


def reference_meters(data, pred, setting):
    args = SimpleNamespace(num_frames=2, **SETTINGS[setting])
    meters = {f"{c}_{k:d}": utils_eval.AverageMeter() for c in CLASSES for k in range(3)}     # main.py:173-180
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        utils_eval.calculate_metrics(args, dict(data), pred, meters)
    names = list(meters)
    ndata = np.array([len(meters[n].epe_data) for n in names], dtype=np.int64)
    return dict(num=np.array([float(meters[n].num) for n in names]), ndata=ndata,
                avg=np.array([[float(getattr(meters[n], m + "_avg")) for m in METRICS] for n in names]),
                data=np.array([[float(getattr(meters[n], m + "_data")[0]) if ndata[i] else 0.0 for m in METRICS] for i, n in enumerate(names)]),
                num_data=np.array([float(meters[n].num_data[0]) if ndata[i] else 0.0 for i, n in enumerate(names)])), names


def near(values, threshold, margin):
    return bool((np.abs(values - threshold) <= margin * abs(threshold)).any())


def margin_ok(gt, pred, rows):
    """the MARGIN CONDITIONS of the module docstring, on the reference's own numbers (`rows`: frame 1)"""
    norm = np.linalg.norm(gt[rows], axis=-1)
    if near(norm.astype(np.float64), 0.05, 1e-6):
        return False
    e = np.linalg.norm(gt[rows] - pred[rows], axis=-1)
    r = e / (np.linalg.norm(gt[rows], axis=-1) + 1e-20)
    return not any(near(e, t, 1e-9) or near(r, t, 1e-9) for t in (0.05, 0.1, 0.3))


def margins(gt, pred, rows):
    norm = np.linalg.norm(gt[rows], axis=-1).astype(np.float64)
    e = np.linalg.norm(gt[rows] - pred[rows], axis=-1)
    r = e / (np.linalg.norm(gt[rows], axis=-1) + 1e-20)
    rel = lambda v, t: float(np.abs(v - t).min() / t)       # noqa: E731
    return rel(norm, 0.05), min(rel(e, t) for t in (0.05, 0.1, 0.3)), min(rel(r, t) for t in (0.05, 0.1, 0.3))


def make_file(seed, kind, background):
    """-> the file-form arrays of one synthetic sample"""
    rng = np.random.default_rng(15_000_003 + seed)
    ftype = np.float64 if kind == "f64" else np.float32
    grid = 2.0 ** 20 if kind == "f64" else 2.0 ** 8

    def cloud():
        p = np.stack([rng.uniform(-40, 40, N), rng.uniform(-40, 40, N), rng.uniform(-0.5, 2.0, N)], axis=1)
        return (np.round(p * grid) / grid).astype(ftype)

    pc1, pc2 = cloud(), cloud()
    values = list(background) + [-1] + list(FOREGROUND)
    cls = np.array([values[k % len(values)] for k in range(N)])
    moving = (np.arange(N) // len(values)) % 2 == 1                # every class value: static rows and dynamic rows
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    flow = (d * np.where(moving, rng.uniform(0.06, 1.5, N), rng.uniform(0.0, 0.04, N))[:, None]).astype(ftype)
    keep1, keep2 = rng.random(N) < 0.7, rng.random(N) < 0.75
    pc1[~keep1], pc2[~keep2], flow[~keep1] = np.nan, np.nan, np.nan
    if kind == "f32_int":
        classes = np.where(keep1, cls, 99).astype(np.int8)
    else:
        classes = np.where(keep1, cls, np.nan).astype(ftype)
    valid = (lambda k: k) if kind == "f32_float" else np.flatnonzero
    return dict(pc1=pc1, pc2=pc2, gt_flow_0_1=flow, pc1_classes=classes, pc2_classes=np.full(N, -1, np.int8),
                ground1=np.zeros(N, np.uint8), ground2=np.zeros(N, np.uint8),
                pc1_flows_valid_idx=valid(keep1), pc2_flows_valid_idx=valid(keep2))


def predicted_flow(seed, gt, rows):
    rng = np.random.default_rng(15_100_003 + seed)
    d = rng.normal(size=gt.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pred = (gt + d * rng.uniform(0.0, 0.5, size=(len(gt), 1))).astype(np.float32)
    pred[~rows] = 0.0                               # main.py:218
    return pred


def record(out, data, pred):
    for setting in SETTINGS:
        rec, names = reference_meters(data, pred, setting)
        out.update({f"{setting}_{k}": v for k, v in rec.items()})
    out["meter_names"] = np.array(names)


def build_synthetic(base_seed, kind):
    _, background = reference_load(make_file(base_seed, kind, (5,)))
    for seed in range(base_seed, base_seed + 100):
        arrays = make_file(seed, kind, background)
        data, _ = reference_load(arrays)
        rows = data["time_indice"] == 1
        pred = predicted_flow(seed, data["scene_flow"], rows)
        if margin_ok(data["scene_flow"], pred, rows):
            break
    else:
        raise SystemExit("no seed meets the margin conditions")
    sd, fb = data["sd_labels"][rows] == 1, data["fb_labels"][rows] == 1
    assert all(x.any() for x in (sd & fb, sd & ~fb, ~sd & fb, ~sd & ~fb)), "static, dynamic, fg and bg all have members"
    out = dict(arrays, pred_flow=pred, background_idxes=background, seed=np.array(seed))
    out.update({"ref_" + k: data[k] for k in SAMPLE_KEYS})
    record(out, data, pred)
    print(f"  {kind}: seed {seed}, m = {len(rows)}, margins (|flow|, e, r) = {margins(data['scene_flow'], pred, rows)}")
    return out


def build_demo():
    path = os.path.join(REF, "demo.npz")
    g8 = np.load(os.path.join(OUT, "g8_demo.npz"))
    with np.load(path) as z:
        v1, v2 = z["pc1_flows_valid_idx"], z["pc2_flows_valid_idx"]
        assert np.array_equal(z["pc1"][v1], g8["point_src"]) and np.array_equal(z["pc2"][v2], g8["point_dst"])
        assert np.array_equal(z["gt_flow_0_1"][v1], g8["gt_flow"])
        classes = z["pc1_classes"][v1]
    assert np.array_equal(classes.astype(np.int8), classes)
    data, background = reference_load(path, "demo")
    rows = data["time_indice"] == 1
    assert np.array_equal(data["raw_points"][rows], g8["point_src"]) and np.array_equal(data["scene_flow"][rows], g8["gt_flow"].astype(np.float64))
    pred = np.concatenate([np.zeros((int((~rows).sum()), 3), np.float32), g8["flow"]])
    assert margin_ok(data["scene_flow"], pred, rows), margins(data["scene_flow"], pred, rows)
    out = dict(classes_valid=classes.astype(np.int8), background_idxes=background,
               ref_sd_labels=data["sd_labels"].astype(np.uint8), ref_fb_labels=data["fb_labels"].astype(np.uint8))
    assert np.array_equal(out["ref_sd_labels"], data["sd_labels"]) and np.array_equal(out["ref_fb_labels"], data["fb_labels"])
    record(out, data, pred)
    sd, fb = data["sd_labels"][rows] == 1, data["fb_labels"][rows] == 1
    print(f"  demo: m = {len(rows)}, dynamic {int(sd.sum())} (fg {int((sd & fb).sum())}), static fg {int((~sd & fb).sum())}, "
          f"margins (|flow|, e, r) = {margins(data['scene_flow'], pred, rows)}, classes {np.unique(classes)}")
    return out


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, generator=np.array("tools/gen_golden_argo.py"), numpy_version=np.array(np.__version__), **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path}  ({size / 1024:.1f} KiB)")
    return size


def main():
    total = save("g15_argo_demo", build_demo())
    for base, kind in ((100, "f32_int"), (200, "f32_float"), (300, "f64")):
        total += save("g15_argo_" + kind, build_synthetic(base, kind))
    assert total < 300 * 1000, total
    print(f"{total / 1024:.1f} KiB in all")


if __name__ == "__main__":
    main()

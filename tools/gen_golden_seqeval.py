#!/usr/bin/env python3
"""Generate tests/golden/g13_seqeval_*.npz: the REFERENCE's own ground-truth construction and sequence evaluation
(utils_loading.ego_motion_compensation / reconstruct_sequence, dataset_pca.py:66-69; utils_eval.calculate_metrics,
utils_eval.py:185-368) on small synthetic Waymo / nuScenes-style samples.  Runs only where the reference is (CPU, numpy);
the fixtures hold inputs and recorded results, no reference source text.  Third-party modules the reference imports and
that cannot be installed are the stand-ins of tools/standins, as for tools/gen_golden.py.

The samples extend icp_flow_amd.synthetic.make_sequence's idea (ego vehicle along x, vehicle-like shells with constant
velocity and yaw rate, static background) by what the evaluation reads: inst_labels, bbox_tsfm [K,F,4,4] (instance k at
time t -> time 0, in frame-0 coordinates; instance 0 is the background), sd_labels (1 = moving), fb_labels (1 = object),
a few rows labelled neither 0 nor 1, points outside the crop and below z_min, and a predicted flow = ground truth + noise
of 0 .. 0.5 m so that every predicate has members on both sides.

Files: g13_seqeval_f{3,5}_{f32,f64}.npz (raw_points stored as float32 / float64; the float32 file's points are the float64
file's rounded) and g13_seqeval_edge.npz (two small sequences: no dynamic_fg point; no static point).  Per file and per
eval_ground in (0, 1): every meter's num, *_avg, *_data after one calculate_metrics call.

MARGIN CONDITION (asserted here, re-asserted by tests/test_seqeval.py from the stored values): no point's error e or
relative error r lies within 1e-9 (relative) of a predicate threshold, and no coordinate within 1e-9 (relative) of a crop
bound -- so a last-bit difference in e, r or the ground truth cannot move a point across.  The seed of a case is the first
one, counting up from its base, for which the reference's own numbers meet the condition.

g13_seqeval_rows.npz is of another kind: the hand-built rows of tests/eval_rows_cases.py, which stand ON the thresholds and
the crop faces or one step off them, with the reference's own verdict -- compute_epe_test on one row at a time (its five
numbers are then that row's e and its four flags), crop_data's kept rows, and calculate_metrics' meters for an F = 3
arrangement of the rows with float64 and with float32 points.  The predicate rows are judged twice: with the float64
scene_flow every other fixture stores, and with scene_flow rounded to float32, where the reference subtracts, takes the
norm and compares in float32.  THE MARGIN CONDITION DOES NOT APPLY TO THIS FILE: being on the margin is its purpose.

Usage:  python tools/gen_golden_seqeval.py          every file
        python tools/gen_golden_seqeval.py rows     g13_seqeval_rows.npz alone
"""
import contextlib
import io
import os
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "tools", "standins"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402

import utils_eval  # noqa: E402  (reference)
import utils_loading  # noqa: E402  (reference)

import eval_rows_cases as ec  # noqa: E402  (tests/)
from icp_flow_amd.synthetic import _shell_points  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CLASSES = ("overall", "static", "static_bg", "static_fg", "dynamic", "dynamic_fg")
METRICS = ("epe", "accs", "accr", "outlier", "Routlier")
CROP = dict(range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
MARGIN = 1e-9
E_THRESHOLDS, R_THRESHOLDS = (0.05, 0.1, 0.3), (0.05, 0.1, 0.3)


def rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_sample(seed, num_frames, n_objects=10, n_min=60, n_max=600, speed=1.2, n_background=1500, noise=0.01, labels="mixed"):
    """-> dict(raw64 [m,3], time_indice, inst_labels, bbox_tsfm, ego_motion_gt, sd_labels, fb_labels)"""
    rng = np.random.default_rng(13_000_003 + seed)
    side = int(np.ceil(np.sqrt(n_objects)))
    objs = []
    for k in range(n_objects):
        n = int(round(np.exp(rng.uniform(np.log(n_min), np.log(n_max)))))
        ext = np.array([rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.0)])
        centre = np.array([(k % side - side / 2) * 12.0 + rng.uniform(-2, 2), (k // side - side / 2) * 12.0 + rng.uniform(-2, 2),
                           rng.uniform(0.5, 1.2)])
        heading = rng.uniform(-np.pi, np.pi)
        moving = rng.uniform() < 0.6
        vel = rng.uniform(0.3, 1.0) * speed * np.array([np.cos(heading), np.sin(heading), 0.0]) * moving
        yaw_rate = np.deg2rad(rng.uniform(-1.5, 1.5)) * moving
        objs.append((_shell_points(rng, ext, n) @ rz(heading).T, centre, vel, yaw_rate, moving))
    span = side * 6.0 + 10.0                       # (34 m for ten objects: some background lies outside the 32 m crop)
    bg = np.stack([rng.uniform(-span, span, n_background), rng.uniform(-span, span, n_background),
                   rng.uniform(-0.2, 1.0, n_background)], axis=1)      # (z_min = 0.3: part of it is 'ground')
    ego_v = np.array([rng.uniform(0.5, 1.5), rng.uniform(-0.1, 0.1), 0.0])
    ego_yaw = np.deg2rad(rng.uniform(-0.8, 0.8))
    K = n_objects + 1
    bbox = np.tile(np.eye(4), (K, num_frames, 1, 1))
    poses = np.tile(np.eye(4), (num_frames, 1, 1))
    raw, tim, inst, sd, fb = [], [], [], [], []
    for j in range(num_frames):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = rz(ego_yaw * j), ego_v * j
        poses[j] = P
        Pinv = np.linalg.inv(P)
        parts, ids, sds, fbs = [], [], [], []
        for k, (local, centre, vel, yaw_rate, moving) in enumerate(objs):
            R = rz(yaw_rate * j)
            bbox[k + 1, j, :3, :3] = R.T                                   # world at time j -> world at time 0
            bbox[k + 1, j, :3, 3] = centre - R.T @ (centre + vel * j)
            keep = rng.random(len(local)) < 0.9
            n = int(keep.sum())
            parts.append(local[keep] @ R.T + centre + vel * j + rng.normal(0.0, noise, size=(n, 3)))
            ids.append(np.full(n, k + 1))
            sds.append(np.full(n, int(moving)))
            # (object 1: labelled background although it is an object, so that `dynamic` / `static` are more than their _fg parts)
            fbs.append(np.full(n, 0 if k == 1 else 1))
        parts.append(bg + rng.normal(0.0, noise, size=bg.shape))
        ids.append(np.zeros(len(bg), int)); sds.append(np.zeros(len(bg), int)); fbs.append(np.zeros(len(bg), int))
        w = np.concatenate(parts)
        r = w @ Pinv[:3, :3].T + Pinv[:3, 3]
        perm = rng.permutation(len(r))
        raw.append(r[perm]); tim.append(np.full(len(r), j))
        inst.append(np.concatenate(ids)[perm]); sd.append(np.concatenate(sds)[perm]); fb.append(np.concatenate(fbs)[perm])
    sd, fb = np.concatenate(sd).astype(np.int64), np.concatenate(fb).astype(np.int64)
    if labels == "mixed":
        odd = rng.random(len(sd)) < 0.01           # unlabelled rows: neither 0 nor 1, counted in `overall` only
        sd[odd] = -1
        odd = rng.random(len(fb)) < 0.01
        fb[odd] = 2
    elif labels == "no_dynamic_fg":
        fb[sd == 1] = 0
    elif labels == "no_static":
        sd[:] = 1
    # 2^-20 m grid: 26 significant bits at 32 m, so rounding to float32 is a real rounding, and the float64 file stays small
    raw64 = np.round(np.concatenate(raw) * 2.0 ** 20) / 2.0 ** 20
    return dict(raw64=raw64, time_indice=np.concatenate(tim).astype(np.int64), inst_labels=np.concatenate(inst).astype(np.int64),
                bbox_tsfm=bbox, ego_motion_gt=poses, sd_labels=sd, fb_labels=fb)


def reference_scene_flow(raw, s, num_frames):
    """dataset_pca.py:66-69, the reference's own functions"""
    ego = utils_loading.ego_motion_compensation(raw, s["time_indice"], s["ego_motion_gt"])
    full = utils_loading.reconstruct_sequence(ego, s["time_indice"], s["inst_labels"], s["bbox_tsfm"], num_frames)
    return full - raw


def predicted_flow(seed, gt, time_indice):
    rng = np.random.default_rng(13_100_003 + seed)
    d = rng.normal(size=gt.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pred = (gt + d * rng.uniform(0.0, 0.5, size=(len(gt), 1))).astype(np.float32)
    pred[time_indice == 0] = 0.0                    # main.py:218
    return pred


def near(values, threshold):
    return bool((np.abs(values - threshold) <= MARGIN * abs(threshold)).any())


def margin_ok(raw, gt, pred):
    """the MARGIN CONDITION of the module docstring, on the reference's own numbers"""
    e = np.linalg.norm(gt - pred, axis=-1)
    r = e / (np.linalg.norm(gt, axis=-1) + 1e-20)
    if any(near(e, t) for t in E_THRESHOLDS) or any(near(r, t) for t in R_THRESHOLDS):
        return False
    raw = raw.astype(np.float64)
    zmin = CROP["range_z"] + CROP["ground_slack"]
    for col, bound in ((np.abs(raw[:, 0]), CROP["range_x"]), (np.abs(raw[:, 1]), CROP["range_y"]), (raw[:, 2], zmin)):
        if near(col, bound) or near(col, float(np.float32(bound))):
            return False
    return True


def reference_meters(raw, s, gt, pred, num_frames, eval_ground, crop=None):
    args = SimpleNamespace(num_frames=num_frames, eval_ground=bool(eval_ground), **(CROP if crop is None else crop))
    meters = {f"{c}_{k:d}": utils_eval.AverageMeter() for c in CLASSES for k in range(num_frames + 1)}    # main.py:173-180
    data = dict(raw_points=raw, time_indice=s["time_indice"], sd_labels=s["sd_labels"], fb_labels=s["fb_labels"],
                ego_motion_gt=s["ego_motion_gt"], scene_flow=gt, data_path="")
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        utils_eval.calculate_metrics(args, data, pred, meters)
    names = list(meters)
    num = np.array([float(meters[n].num) for n in names])
    ndata = np.array([len(meters[n].epe_data) for n in names], dtype=np.int64)
    avg = np.array([[float(getattr(meters[n], m + "_avg")) for m in METRICS] for n in names])
    data_ = np.array([[float(getattr(meters[n], m + "_data")[0]) if ndata[i] else 0.0 for m in METRICS] for i, n in enumerate(names)])
    wts = np.array([float(meters[n].num_data[0]) if ndata[i] else 0.0 for i, n in enumerate(names)])
    return dict(num=num, ndata=ndata, avg=avg, data=data_, num_data=wts), names


def build_case(base_seed, num_frames, dtype, **kw):
    for seed in range(base_seed, base_seed + 100):
        s = make_sample(seed, num_frames, **kw)
        ok = True
        for dt in (np.float32, np.float64):        # (both files of a pair come from one seed)
            raw = s["raw64"].astype(dt)
            gt = reference_scene_flow(raw, s, num_frames)
            ok = ok and margin_ok(raw, gt, predicted_flow(seed, gt, s["time_indice"]))
        if ok:
            break
    else:
        raise SystemExit("no seed meets the margin condition")
    raw = s["raw64"].astype(dtype)
    gt = reference_scene_flow(raw, s, num_frames)
    assert gt.dtype == np.float64
    pred = predicted_flow(seed, gt, s["time_indice"])
    assert margin_ok(raw, gt, pred)
    out = dict(raw_points=raw, time_indice=s["time_indice"], inst_labels=s["inst_labels"], bbox_tsfm=s["bbox_tsfm"],
               ego_motion_gt=s["ego_motion_gt"], sd_labels=s["sd_labels"], fb_labels=s["fb_labels"], scene_flow=gt, pred_flow=pred,
               num_frames=np.array(num_frames), seed=np.array(seed), **{k: np.array(v) for k, v in CROP.items()})
    for g in (0, 1):
        rec, names = reference_meters(raw, s, gt, pred, num_frames, g)
        out.update({f"eg{g}_{k}": v for k, v in rec.items()})
    out["meter_names"] = np.array(names)
    return out


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, generator=np.array("tools/gen_golden_seqeval.py"), numpy_version=np.array(np.__version__), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f"wrote {path}  ({size / 1024:.1f} KiB)")


def reference_rows(gt, pred):
    """compute_epe_test on one row at a time -> (e [n] in the type the reference computed it in, flags uint8 [n,4])"""
    e, flags = [], []
    with np.errstate(all="ignore"):
        for k in range(len(gt)):
            out = utils_eval.compute_epe_test(pred[k:k + 1], gt[k:k + 1])
            e.append(out[0])
            flags.append([int(v) for v in out[1:]])
            assert all(v in (0.0, 1.0) for v in out[1:])
    return np.array(e), np.array(flags, dtype=np.uint8)


def reference_keep(pts, eval_ground=False):
    """the rows crop_data keeps, read off an index array sent through it in the place of the labels"""
    n = len(pts)
    args = SimpleNamespace(eval_ground=eval_ground, range_x=ec.RANGE_X, range_y=ec.RANGE_Y, range_z=ec.RANGE_Z, ground_slack=ec.GROUND_SLACK)
    data = dict(raw_points=pts, time_indice=np.zeros(n, np.int64), sd_labels=np.arange(n), fb_labels=np.zeros(n, np.int64),
                ego_motion_gt=None, scene_flow=np.zeros((n, 3)), data_path="")
    with np.errstate(all="ignore"):
        cropped, _ = utils_eval.crop_data(args, data, np.zeros((n, 3), np.float32))
    keep = np.zeros(n, bool)
    keep[cropped["sd_labels"]] = True
    return keep


def build_rows():
    p = ec.predicate_rows()
    out = dict(pred_name=p.name, pred_gt=p.gt, pred_pred=p.pred)
    out["pred_e"], out["pred_flags"] = reference_rows(p.gt, p.pred)
    gt32 = p.gt.astype(np.float32)
    out["pred32_e"], out["pred32_flags"] = reference_rows(gt32, p.pred)
    assert out["pred_e"].dtype == np.float64 and out["pred32_e"].dtype == np.float32
    for dtype, tag in ((np.float64, "f64"), (np.float32, "f32")):
        c = ec.crop_rows(dtype)
        out[f"crop_{tag}_name"], out[f"crop_{tag}_pts"], out[f"crop_{tag}_keep"] = c.name, c.pts, reference_keep(c.pts)
        out[f"crop_{tag}_keep_xy"] = reference_keep(c.pts, eval_ground=True)        # (crop_data's x-y half, which calculate_metrics never uses alone)
        s = ec.meter_sample(dtype)
        crop = dict(range_x=ec.RANGE_X, range_y=ec.RANGE_Y, range_z=ec.RANGE_Z, ground_slack=ec.GROUND_SLACK)
        prefix = f"m{tag[1:]}__"
        out.update({prefix + k: v for k, v in s.data.items()})
        out[prefix + "pred_flow"], out[prefix + "num_frames"] = s.pred, np.array(s.F)
        out.update({prefix + k: np.array(v) for k, v in crop.items()})
        for g in (0, 1):
            rec, names = reference_meters(s.data["raw_points"], dict(s.data, ego_motion_gt=None), s.data["scene_flow"], s.pred, s.F, g, crop)
            out.update({prefix + f"eg{g}_{k}": v for k, v in rec.items()})
        out[prefix + "meter_names"] = np.array(names)
    return out


def main():
    if sys.argv[1:] == ["rows"]:
        save("g13_seqeval_rows", build_rows())
        return
    save("g13_seqeval_rows", build_rows())
    for F, base in ((3, 300), (5, 500)):
        for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
            c = build_case(base, F, dtype)
            save(f"g13_seqeval_f{F}_{tag}", c)
            print(f"  F={F} {tag}: seed {int(c['seed'])}, m={len(c['raw_points'])}, overall_0 = {c['eg0_avg'][0]}")
    edge = {}
    for label in ("no_dynamic_fg", "no_static"):
        c = build_case(900, 3, np.float64, n_objects=4, n_min=30, n_max=80, n_background=150, labels=label)
        edge.update({f"{label}__{k}": v for k, v in c.items()})
    save("g13_seqeval_edge", edge)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/g14_segments_*.npz: the REFERENCE's own verbose loop -- utils_debug.debug_frame's crop and three
per-frame rows (utils_debug.py:37-61) and utils_flow.flow_evaluation's per-segment numbers and printed lines
(utils_flow.py:72-124) -- on a small labelled synthetic frame pair.  Runs only where the reference is (CPU, numpy, scipy); the
fixtures hold inputs and recorded results, no reference source text.  Third-party modules the reference imports and that
cannot be installed are the stand-ins of tools/standins, as for tools/gen_golden_seqeval.py; its visualisation calls are
replaced by no-ops for the run.

The frame pair: about 3 000 + 3 000 points, rows interleaved; labels -1e8 (ground), -1 (noise) and 12 clusters with
non-contiguous ids; 8 clusters matched by [P,10] pair rows (one of them to a destination cluster of another id), 4 not; two
clusters absent from the destination cloud; cluster 57 predicted 3 m off (EPE > 2 m: the reference's "substantially large flow
errors" block); cluster 23 entirely below z_min; predicted flow = ground truth + noise of 0 .. 0.5 m.

Files: g14_segments_{f32,f64}.npz (points stored as float32 / float64; the float32 file's points are the float64 file's
rounded).  Per file, with the z crop of utils_debug.py:37-46 ("crop_") and without ("all_"): per segment of
np.unique(src_labels) the five numbers of the reference's compute_epe_test on the masks of utils_flow.py:88-95, len_i,
len_j, the means, mean(x + flow) and the translation norm; scipy's as_euler("zyx", degrees=True) of every transform; the
three debug_frame rows; the text the reference's flow_evaluation printed.

MARGIN CONDITION (asserted here, re-asserted by tests/test_segments.py from the stored values): no row's e or r lies within
1e-9 (relative) of a predicate threshold, no z within 1e-9 of z_min (as given and as rounded to float32), and no segment's EPE
within 1e-9 of 2.0.  The seed is the first one, counting up from its base, for which the reference's numbers meet it.

Usage:  python tools/gen_golden_segments.py
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

import matplotlib  # noqa: E402

matplotlib.use("Agg")
import numpy as np  # noqa: E402
from scipy.spatial.transform import Rotation  # noqa: E402

import utils_debug as ref_debug  # noqa: E402  (the reference's modules, under names of their own: the package has modules of the same names)
import utils_eval as ref_eval  # noqa: E402
import utils_flow as ref_flow  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
MARGIN = 1e-9
THRESHOLDS = (0.05, 0.1, 0.3)
CROP = dict(range_z=0.0, ground_slack=0.3)
Z_MIN = CROP["range_z"] + CROP["ground_slack"]
CLUSTERS = (0, 2, 3, 7, 11, 12, 19, 23, 40, 57, 199, 310)
MATCHED = (0, 2, 7, 11, 19, 57, 199, 310)
REMATCHED = {11: 12}            # source cluster 11 is matched to destination cluster 12
ABSENT_IN_DST = (3, 40)
FAR_OFF, BELOW = 57, 23
GROUND, NOISE = -1e8, -1.0


def rigid(rng, max_deg, max_t):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("zyx", rng.uniform(-max_deg, max_deg, 3), degrees=True).as_matrix()
    T[:3, 3] = rng.uniform(-max_t, max_t, 3) * np.array([1.0, 1.0, 0.1])
    return T


def make_pair(seed):
    rng = np.random.default_rng(14_000_003 + seed)
    pose = rigid(rng, 1.0, 1.0)
    src, dst, ls, ld, gt, sd, fb, motion = [], [], [], [], [], [], [], {}
    for k, cid in enumerate(CLUSTERS):
        n_i, n_j = int(rng.integers(40, 400)), int(rng.integers(40, 400))
        centre = np.array([rng.uniform(-30, 30), rng.uniform(-30, 30), rng.uniform(0.9, 1.6)])
        ext = np.array([rng.uniform(1.5, 4.5), rng.uniform(1.0, 2.0), rng.uniform(0.8, 1.0)])
        if cid == BELOW:
            centre[2], ext[2] = 0.0, 0.4                       # z in [-0.2, 0.2]: every row below z_min = 0.3
        moving = k % 3 != 0
        T = rigid(rng, 8.0, 1.5) if moving else np.eye(4)
        motion[cid] = T
        x = centre + rng.uniform(-0.5, 0.5, (n_i, 3)) * ext
        full = T @ pose
        src.append(x); ls.append(np.full(n_i, float(cid)))
        gt.append(x @ full[:3, :3].T + full[:3, 3] - x)
        sd.append(np.full(n_i, int(moving))); fb.append(np.ones(n_i, int))
        if cid not in ABSENT_IN_DST:
            y = centre + rng.uniform(-0.5, 0.5, (n_j, 3)) * ext
            dst.append(y @ full[:3, :3].T + full[:3, 3]); ld.append(np.full(n_j, float(cid)))
    for lab, n_i, n_j, zlo, zhi in ((GROUND, 900, 800, -0.2, 0.6), (NOISE, 300, 350, 0.0, 2.5)):
        for n, pts, labs in ((n_i, src, ls), (n_j, dst, ld)):
            x = np.stack([rng.uniform(-32, 32, n), rng.uniform(-32, 32, n), rng.uniform(zlo, zhi, n)], axis=1)
            pts.append(x); labs.append(np.full(n, lab))
            if pts is src:
                gt.append(x @ pose[:3, :3].T + pose[:3, 3] - x)
                sd.append(np.zeros(n, int)); fb.append(np.zeros(n, int))
    src, dst, ls, ld = np.concatenate(src), np.concatenate(dst), np.concatenate(ls), np.concatenate(ld)
    gt, sd, fb = np.concatenate(gt), np.concatenate(sd), np.concatenate(fb)
    d = rng.normal(size=gt.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pred = gt + d * rng.uniform(0.0, 0.5, size=(len(gt), 1))
    pred[ls == FAR_OFF] += np.array([2.5, -1.5, 0.5])
    pi, pj = rng.permutation(len(src)), rng.permutation(len(dst))           # rows interleaved, not grouped by label
    src, ls, gt, sd, fb, pred = src[pi], ls[pi], gt[pi], sd[pi], fb[pi], pred[pi].astype(np.float32)
    dst, ld = dst[pj], ld[pj]
    # 2^-20 m grid: rounding to float32 is a real rounding and the float64 file stays small
    src, dst = np.round(src * 2.0 ** 20) / 2.0 ** 20, np.round(dst * 2.0 ** 20) / 2.0 ** 20
    pairs = np.zeros((len(MATCHED), 10))
    for row, cid in enumerate(MATCHED):
        pairs[row, 0], pairs[row, 1] = cid, REMATCHED.get(cid, cid)
        pairs[row, 2:] = rng.uniform(0.0, 1.0, 8)
    order = rng.permutation(len(MATCHED))
    pairs = pairs[order]
    transformations = np.stack([motion[int(c)] for c in pairs[:, 0]])
    return dict(src64=src, dst64=dst, src_labels=ls, dst_labels=ld, flow_gt=gt, flow_pd=pred, sd_label=sd.astype(np.int64),
                fb_label=fb.astype(np.int64), pose=pose, pairs=pairs, transformations=transformations)


def near(values, threshold):
    return bool((np.abs(values - threshold) <= MARGIN * abs(threshold)).any())


def margin_ok(src, gt, pred, seg_epe):
    e = np.linalg.norm(gt - pred, axis=-1)
    r = e / (np.linalg.norm(gt, axis=-1) + 1e-20)
    if any(near(e, t) or near(r, t) for t in THRESHOLDS):
        return False
    z = src[:, 2].astype(np.float64)
    if near(z, Z_MIN) or near(z, float(np.float32(Z_MIN))):
        return False
    return not near(seg_epe[~np.isnan(seg_epe)], 2.0)


def crop(c, src, dst, on):
    """utils_debug.py:37-46: the source rows with z above the threshold, numpy's own comparison for the array's dtype"""
    keep = src[:, 2] > CROP["range_z"] + CROP["ground_slack"] if on else np.ones(len(src), bool)
    return dict(src=src[keep], dst=dst, src_label=c["src_labels"][keep], dst_label=c["dst_labels"], flow=c["flow_pd"][keep],
                flow_gt=c["flow_gt"][keep], sd=c["sd_label"][keep], fb=c["fb_label"][keep])


def reference_segments(c, v):
    """the numbers of utils_flow.py:86-95, 110, 123 per segment, by the reference's own compute_epe_test and numpy expressions"""
    unqs = np.unique(v["src_label"].astype(int))
    rec = {k: [] for k in ("epe", "accs", "accr", "outlier", "routlier", "len_i", "len_j", "mean_i", "mean_j", "moved", "translation")}
    with np.errstate(all="ignore"):
        for unq in unqs:
            idx_i, idx_j = v["src_label"] == unq, v["dst_label"] == unq
            xyz_i, xyz_j = v["src"][idx_i, 0:3], v["dst"][idx_j, 0:3]
            fp, fg = v["flow"][idx_i], v["flow_gt"][idx_i]
            m = ref_eval.compute_epe_test(fp, fg)
            for name, val in zip(("epe", "accs", "accr", "outlier", "routlier"), m):
                rec[name].append(float(val))
            rec["len_i"].append(len(xyz_i)); rec["len_j"].append(len(xyz_j))
            rec["mean_i"].append(xyz_i.mean(0).astype(np.float64)); rec["mean_j"].append(xyz_j.mean(0).astype(np.float64))
            moved = (xyz_i + fp).mean(0)
            rec["moved"].append(moved.astype(np.float64))
            rec["translation"].append(float(np.linalg.norm(moved - xyz_i.mean(0))))
    out = {k: np.array(val) for k, val in rec.items()}
    out["labels"] = unqs.astype(np.int64)
    return out


def reference_frame_rows(v):
    """utils_debug.py:48-61 by the reference's compute_epe_test: rows overall, static, dynamic (NaN row when it has no point)"""
    rows = []
    with np.errstate(all="ignore"):
        for mask in (None, v["sd"] == 0, v["sd"] == 1):
            if mask is not None and not mask.any():
                rows.append([np.nan] * 5 + [0.0])
                continue
            m = ref_eval.compute_epe_test(v["flow"], v["flow_gt"], mask)
            rows.append([float(x) for x in m] + [float(len(v["flow"]) if mask is None else mask.sum())])
    return np.array(rows)


def reference_text(c, v, on):
    """what the reference's debug_frame and flow_evaluation print on this frame pair (its visualisation replaced by no-ops)"""
    nop = lambda *a, **k: None    # noqa: E731
    args = SimpleNamespace(num_frames=2, eval_ground=not on, **CROP)
    result = dict(j=1, dst=v["dst"], src=np.asarray(c["_src"]), pose=c["pose"], sd_label=c["sd_label"], fb_label=c["fb_label"],
                  scene_flow=c["flow_gt"], src_label=c["src_labels"], dst_label=c["dst_labels"], flow=c["flow_pd"])
    ref_debug.visualize_pcd = nop
    ref_flow.visualize_pcd_multiple = nop
    frame, seg = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(frame), np.errstate(all="ignore"):
        ref_debug.debug_frame(args, result)
    with contextlib.redirect_stdout(seg), np.errstate(all="ignore"):
        ref_flow.flow_evaluation(v["src"], v["dst"], v["src_label"], v["dst_label"], v["flow"], v["flow_gt"], c["pose"],
                                   c["transformations"], pairs=c["pairs"])
    return frame.getvalue(), seg.getvalue()


def build_case(base_seed, dtype):
    for seed in range(base_seed, base_seed + 100):
        c = make_pair(seed)
        ok = True
        for dt in (np.float32, np.float64):
            src = c["src64"].astype(dt)
            for on in (True, False):
                seg = reference_segments(c, crop(c, src, c["dst64"].astype(dt), on))
                ok = ok and margin_ok(src, c["flow_gt"], c["flow_pd"], seg["epe"])
        if ok:
            break
    else:
        raise SystemExit("no seed meets the margin condition")
    src, dst = c["src64"].astype(dtype), c["dst64"].astype(dtype)
    c["_src"] = src
    out = dict(src_points=src, dst_points=dst, src_labels=c["src_labels"].astype(np.float32), dst_labels=c["dst_labels"].astype(np.float32),
               flow_gt=c["flow_gt"], flow_pd=c["flow_pd"], sd_label=c["sd_label"], fb_label=c["fb_label"], pose=c["pose"], pairs=c["pairs"],
               transformations=c["transformations"], seed=np.array(seed), z_min=np.array(Z_MIN),
               **{k: np.array(v) for k, v in CROP.items()})
    c["src_labels"], c["dst_labels"] = out["src_labels"], out["dst_labels"]
    out["euler_zyx_deg"] = np.stack([Rotation.from_matrix(T[0:3, 0:3]).as_euler("zyx", degrees=True) for T in c["transformations"]])
    for on, tag in ((True, "crop_"), (False, "all_")):
        v = crop(c, src, dst, on)
        for k, val in reference_segments(c, v).items():
            out[tag + k] = val
        out[tag + "frame_rows"] = reference_frame_rows(v)
        frame_text, seg_text = reference_text(c, v, on)
        out[tag + "frame_text"], out[tag + "segment_text"] = np.array(frame_text), np.array(seg_text)
    assert out["crop_epe"].max() > 2.0 and BELOW not in out["crop_labels"] and BELOW in out["all_labels"]
    return out


def save(name, arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, generator=np.array("tools/gen_golden_segments.py"), numpy_version=np.array(np.__version__), **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print(f"wrote {path}  ({size / 1024:.1f} KiB)")


def main():
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        c = build_case(140, dtype)
        save(f"g14_segments_{tag}", c)
        print(f"  {tag}: seed {int(c['seed'])}, {len(c['src_points'])} + {len(c['dst_points'])} points, segments {len(c['crop_labels'])} / "
              f"{len(c['all_labels'])}, worst EPE {np.nanmax(c['crop_epe']):.4f}")
        print(str(c["crop_frame_text"]) + "\n".join(str(c["crop_segment_text"]).splitlines()[:4]))


if __name__ == "__main__":
    main()

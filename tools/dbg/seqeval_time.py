#!/usr/bin/env python3
"""ms per sequence of the synthetic F = 5 sample: frame_pairs.run_sequences (flows stay on the device, one table read-back)
against the same sample through the path that existed before (every frame pair's flow read back, the reference's metric
table in numpy on the host).  The registration is the same in both; the difference is the evaluation.

    python tools/dbg/seqeval_time.py [--repeat 5] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from icp_flow_amd import frame_pairs, synthetic, utils_eval   # noqa: E402


def host_table(args, sample, flows, meters):
    """the reference's calculate_metrics restated with the package's host functions (crop, masks, compute_epe_test per row)"""
    data, pred = utils_eval.crop_data(args, sample, flows) if not args.eval_ground else (sample, flows)
    t, sd, fb, gt = data["time_indice"], data["sd_labels"], data["fb_labels"], data["scene_flow"]
    masks = lambda s, f: (None, s == 0, (s == 0) & (f == 0), (s == 0) & (f == 1), s == 1, (s == 1) & (f == 1))   # noqa: E731
    for j in list(range(1, args.num_frames)) + [0, args.num_frames]:
        sel = (t == j) if 1 <= j < args.num_frames else (t > 0)
        for c, mask in enumerate(masks(sd[sel], fb[sel])):
            n = int(sel.sum()) if mask is None else int(mask.sum())
            if c >= 2 and n == 0:
                continue
            vals = utils_eval.compute_epe_test(pred[sel], gt[sel], mask)
            meters[f"{utils_eval.METRIC_CLASSES[c]}_{j}"].update(*vals, 1 if j == args.num_frames else len(pred) if (j, c) == (0, 0) else n)
    return meters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    d = synthetic.make_sequence(seed=1, num_frames=5)
    sd = (d["nonground"] & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "val"))
    path = os.path.join(tmp, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=d["nonground"].astype(np.int64))
    a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 5, 0.0, 0.05, False, "ego_motion_gt"
    ours, ours_eval, old, old_eval = [], [], [], []
    for k in range(ns.repeat + 1):
        res = frame_pairs.run_sequences(a, [path], dev)
        sample = frame_pairs.load_sequence_sample(path, a)
        fps = frame_pairs.load_sequence(path, a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flows = np.zeros((len(sample["raw_points"]), 3), np.float32)
        for fp in fps:
            flows[sample["time_indice"] == fp.gap] = frame_pairs.register_frame_pair(a, fp, dev)["flow"].cpu().numpy()
        t1 = time.perf_counter()
        meters = host_table(a, sample, flows, utils_eval.new_metric_table(5))
        t2 = time.perf_counter()
        if k:                        # (the first pass pays for allocations and page-in)
            ours.append(res["ms_per_sequence"]); ours_eval.append(res["ms_eval_per_sequence"])
            old.append((t2 - t0) * 1e3); old_eval.append((t2 - t1) * 1e3)
        assert abs(meters["overall_0"].epe_avg - res["metrics"]["overall_0"].epe_avg) < 1e-9
    med = lambda v: float(np.median(v))   # noqa: E731
    out = dict(points=int(len(d["raw_points"])), frames=5, repeat=ns.repeat,
               device_table_ms_per_sequence=med(ours), device_table_eval_ms=med(ours_eval),
               readback_numpy_ms_per_sequence=med(old), readback_numpy_eval_ms=med(old_eval),
               overall_0_epe=float(res["metrics"]["overall_0"].epe_avg))
    print(json.dumps(out))
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

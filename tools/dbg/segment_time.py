#!/usr/bin/env python3
"""ms per frame pair of the per-segment report (utils_debug.debug_frame + utils_flow.flow_evaluation: icpflow_seq_metrics with
two frames, icpflow_seq_segment_table on both clouds, one read-back, the host half) on the synthetic F = 5 sample, next to
ms_eval_per_sequence of the same run for scale.

    python tools/dbg/segment_time.py [--repeat 5] [--out FILE.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from icp_flow_amd import frame_pairs, synthetic   # noqa: E402


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
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source, a.if_verbose = 5, 0.0, 0.05, False, "ego_motion_gt", True
    report, evaluation, segments = [], [], 0
    for k in range(ns.repeat + 1):
        with contextlib.redirect_stdout(io.StringIO()):
            res = frame_pairs.run_sequences(a, [path], dev)
        if k:                        # (the first pass pays for allocations and page-in)
            report.append(res["ms_report_per_sequence"] / res["frame_pairs"])
            evaluation.append(res["ms_eval_per_sequence"])
        segments = sum(len(r["segments"]) for r in res["segments"])
    med = lambda v: float(np.median(v))   # noqa: E731
    out = dict(points=int(len(d["raw_points"])), frames=5, frame_pairs=int(res["frame_pairs"]), segments=int(segments), repeat=ns.repeat,
               report_ms_per_frame_pair=med(report), ms_eval_per_sequence=med(evaluation))
    print(json.dumps(out))
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

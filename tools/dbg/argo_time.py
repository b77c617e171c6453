#!/usr/bin/env python3
"""ms per sample of the Argoverse 2 path on the demo sample (tests/golden/g8_demo.npz's rows in file form, 90 000-row arrays):
the sample construction alone (utils_loading.argo_sample on resident arrays: icpflow_seq_argo_sample and its read-back of the
bad-row count) and frame_pairs.run_sequences(dataset="argo") (registration + evaluation, as it reports them).

    python tools/dbg/argo_time.py [--repeat 10] [--cluster dbscan] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from icp_flow_amd import frame_pairs, utils_loading   # noqa: E402


def demo_file():
    """g8_demo's valid rows scattered into 90 000-row arrays, NaN elsewhere; classes: every row foreground but a tenth"""
    g8 = np.load(os.path.join(REPO, "tests", "golden", "g8_demo.npz"))
    n, rng = 90_000, np.random.default_rng(15)
    m1, m2 = len(g8["point_src"]), len(g8["point_dst"])
    v1, v2 = np.sort(rng.choice(n, m1, replace=False)), np.sort(rng.choice(n, m2, replace=False))
    pc1, pc2, flow = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
    cls = np.full(n, np.nan, np.float32)
    pc1[v1], pc2[v2], flow[v1] = g8["point_src"], g8["point_dst"], g8["gt_flow"]
    cls[v1] = np.where(rng.random(m1) < 0.1, -1.0, 18.0)
    return dict(pc1=pc1, pc2=pc2, gt_flow_0_1=flow, pc1_classes=cls, pc1_flows_valid_idx=v1, pc2_flows_valid_idx=v2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--cluster", default="dbscan", choices=("dbscan", "hdbscan"))
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    arrays = demo_file()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "demo.npz")
    np.savez(path, **arrays)
    resident = {k: torch.from_numpy(v).to(dev) for k, v in arrays.items()}
    build = []
    for k in range(ns.repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        utils_loading.argo_sample(resident["pc1"], resident["pc2"], resident["gt_flow_0_1"], resident["pc1_classes"],
                                  resident["pc1_flows_valid_idx"], resident["pc2_flows_valid_idx"])
        torch.cuda.synchronize()
        if k:                        # (the first pass pays for allocations and page-in)
            build.append((time.perf_counter() - t0) * 1e3)
    a = frame_pairs.default_args(cluster=ns.cluster, speed=1.67, range_x=10000.0, range_y=10000.0)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground = 2, -10000.0, 0.0, False
    runs, evals = [], []
    for k in range(ns.repeat + 1):
        res = frame_pairs.run_sequences(a, [path], dev, dataset="argo")
        if k:
            runs.append(res["ms_per_sequence"]); evals.append(res["ms_eval_per_sequence"])
    med = lambda v: float(np.median(v))   # noqa: E731
    out = dict(points=int(len(arrays["pc1_flows_valid_idx"]) + len(arrays["pc2_flows_valid_idx"])), repeat=ns.repeat, cluster=ns.cluster,
               sample_construction_ms=med(build), run_sequences_ms_per_sample=med(runs), evaluation_ms_per_sample=med(evals),
               overall_0_epe=float(res["metrics"]["overall_0"].epe_avg))
    print(json.dumps(out))
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per sample of the evaluation run_sequences(dataset="argo") times as ms_eval_per_sequence, on the demo sample (126 598 rows:
tests/golden/g8_demo.npz's rows in file form, the sample built on the device, g8's flow as the prediction): without the
class table -- utils_eval.calculate_metrics alone, the path before icpflow_seq_class_table -- and with it, calculate_metrics
followed by utils_eval.class_table, each with its read-back.  The same calls run_sequences makes between its two stamps;
the registration is left out, it is the same on both sides.

    python tools/dbg/class_table_time.py [--repeat 30] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from icp_flow_amd import frame_pairs, utils_eval, utils_loading   # noqa: E402


def demo_sample(dev):
    """-> (the sample on the device, predicted flow float32 [m,3] on the device)"""
    g8 = np.load(os.path.join(REPO, "tests", "golden", "g8_demo.npz"))
    g15 = np.load(os.path.join(REPO, "tests", "golden", "g15_argo_demo.npz"))
    n, rng = 90_000, np.random.default_rng(15)
    m1, m2 = len(g8["point_src"]), len(g8["point_dst"])
    v1, v2 = np.sort(rng.choice(n, m1, replace=False)), np.sort(rng.choice(n, m2, replace=False))
    pc1, pc2, flow = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
    cls = np.full(n, np.nan, np.float32)
    pc1[v1], pc2[v2], flow[v1], cls[v1] = g8["point_src"], g8["point_dst"], g8["gt_flow"], g15["classes_valid"]
    data = utils_loading.argo_sample(pc1, pc2, flow, cls, v1, v2, device=dev)
    pred = torch.from_numpy(np.concatenate([np.zeros((m2, 3), np.float32), g8["flow"]])).to(dev)
    return data, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    data, pred = demo_sample(dev)
    a = frame_pairs.default_args(range_x=10000.0, range_y=10000.0)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground = 2, -10000.0, 0.0, False
    times = {False: [], True: []}
    for k in range(ns.repeat + 1):
        for with_table in (False, True):
            meters = utils_eval.new_metric_table(2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            utils_eval.calculate_metrics(a, data, pred, meters)
            table = utils_eval.class_table(a, data, pred) if with_table else None
            t1 = time.perf_counter()
            if k:                        # (the first pass pays for allocations and page-in)
                times[with_table].append((t1 - t0) * 1e3)
    med = lambda v: float(np.median(v))   # noqa: E731
    tw = table.threeway()
    out = dict(points=int(len(data["time_indice"])), repeat=ns.repeat, device=torch.cuda.get_device_name(dev),
               ms_eval_per_sequence=med(times[False]), ms_eval_per_sequence_with_class_table=med(times[True]),
               class_table_ms=med(times[True]) - med(times[False]), rows_counted=int(table.counts.sum()),
               threeway=dict(mean=tw["mean"], FD=tw["FD"], FS=tw["FS"], BS=tw["BS"]), overall_0_epe=float(meters["overall_0"].epe_avg))
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per sample of the evaluation run_sequences(dataset="argo") times as ms_eval_per_sequence, on the demo sample of
tools/dbg/class_table_time.py (126 598 rows), three ways in one session: utils_eval.calculate_metrics alone (no flag: the path
before either table), followed by utils_eval.class_table (`--class-table meta`), and followed by utils_eval.bucket_table
(`--bucketed-epe`: icpflow_seq_bucket_table, 33 rows x 51 buckets), each with its read-back.  The same calls run_sequences
makes between its two stamps; the registration is left out, it is the same on every side.  Medians of --repeat.

    python tools/dbg/bucket_table_time.py [--repeat 30] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from class_table_time import demo_sample                          # noqa: E402
from icp_flow_amd import frame_pairs, utils_eval                  # noqa: E402

WAYS = ("none", "class_table", "bucket_table")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    data, pred = demo_sample(dev)
    a = frame_pairs.default_args(range_x=10000.0, range_y=10000.0)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground = 2, -10000.0, 0.0, False
    times = {w: [] for w in WAYS}
    table = None
    for k in range(ns.repeat + 1):
        for way in WAYS:
            meters = utils_eval.new_metric_table(2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            utils_eval.calculate_metrics(a, data, pred, meters)
            if way == "class_table":
                utils_eval.class_table(a, data, pred)
            elif way == "bucket_table":
                table = utils_eval.bucket_table(a, data, pred)
            t1 = time.perf_counter()
            if k:                        # (the first pass pays for allocations and page-in)
                times[way].append((t1 - t0) * 1e3)
    med = {w: float(np.median(times[w])) for w in WAYS}
    epe = utils_eval.bucketed_epe(table)
    out = dict(points=int(len(data["time_indice"])), repeat=ns.repeat, device=torch.cuda.get_device_name(dev),
               ms_eval_per_sequence=med["none"], ms_eval_per_sequence_with_class_table=med["class_table"],
               ms_eval_per_sequence_with_bucket_table=med["bucket_table"], class_table_ms=med["class_table"] - med["none"],
               bucket_table_ms=med["bucket_table"] - med["none"], rows_counted=int(table.counts.sum()),
               cells_used=int((table.counts > 0).sum()), mean_static=epe["mean_static"], mean_dynamic=epe["mean_dynamic"])
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

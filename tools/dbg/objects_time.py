#!/usr/bin/env python3
"""ms of the object boxes (icpflow_segment_boxes, icpflow_pair_objects, csrc/boxes.hip) on the demo frame pair of
tests/golden/g8_demo (63 276 source x 63 322 destination points, labels of g8_demo_labels), medians of --repeat, every figure a
host clock around work that ends in a device synchronise, all in one session:

    segment_boxes_ms    icpflow_segment_boxes alone -- its five launches -- on the source cloud, its cluster table resident
    cluster_table_ms    icpflow_cluster_table on the same cloud, which segment_boxes_device runs first when it is given none
    pair_objects_ms     icpflow_pair_objects alone, both box tables resident
    frame_objects_ms    frame_pairs.frame_objects: two cluster tables, two box tables, the pairs' objects and the one read-back
                        -- what `--objects` adds per frame pair
and what the objects of that frame pair are: the counts, the largest centre gap, and, for the rows that carry gt_flow, the
difference between an object's displacement and the mean ground-truth flow of its cluster (host numpy).  Not gated: the calls
are new.

    python tools/dbg/objects_time.py [--repeat 30] [--out profiles/objects_ms.json]
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_golden                                              # noqa: E402
from icp_flow_amd import _lib, frame_pairs, utils_objects                     # noqa: E402


def median_ms(fn, repeat):
    times = []
    for k in range(repeat + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:                            # (the first pass pays for allocations and page-in)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    g, lab = load_golden("g8_demo"), load_golden("g8_demo_labels")
    fp = frame_pairs.FramePair(g["point_src"], g["point_dst"], lab["label_src"], lab["label_dst"], gt_flow=g["gt_flow"], name="g8_demo")
    frame_pairs.make_resident(fp, dev)
    a = frame_pairs.default_args()
    a.objects = True
    registered = frame_pairs.register_frame_pair(a, fp, dev)
    ps, pd = frame_pairs._input(fp, "points_src", dev), frame_pairs._input(fp, "points_dst", dev)
    ls, ld = registered["labels_src"].float().contiguous(), registered["labels_dst"].float().contiguous()
    pairs, T = registered["pairs"], registered["transformations"]
    table = utils_objects.cluster_table_device(ps, ls)
    boxes_src, num_src = utils_objects.segment_boxes_device(ps, ls, table=table)
    boxes_dst, num_dst = utils_objects.segment_boxes_device(pd, ld)

    out = dict(points_src=len(ps), points_dst=len(pd), segments_src=int(num_src.item()), segments_dst=int(num_dst.item()),
               matched_pairs=int(pairs.shape[0]), repeat=ns.repeat, device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO,
               date=datetime.date.today().isoformat(), delta=utils_objects.BOX_DELTA, directions=utils_objects.BOX_DIRECTIONS,
               seconds=utils_objects.SWEEP_SECONDS, min_speed=utils_objects.MIN_SPEED)
    out["cluster_table_ms"] = median_ms(lambda: utils_objects.cluster_table_device(ps, ls), ns.repeat)
    out["segment_boxes_ms"] = median_ms(lambda: utils_objects.segment_boxes_device(ps, ls, table=table), ns.repeat)
    out["pair_objects_ms"] = median_ms(lambda: utils_objects.pair_objects_device(boxes_src, num_src, pairs, T, boxes_dst, num_dst), ns.repeat)
    out["frame_objects_ms"] = median_ms(lambda: frame_pairs.frame_objects(fp, registered, dev), ns.repeat)
    objects = frame_pairs.frame_objects(fp, registered, dev)
    out["counts"] = objects.summary()
    out["largest_centre_gap_m"] = objects.largest_centre_gap()
    listed = objects.as_list()
    gaps = np.array([e["centre_gap"] for e in listed if e["centre_gap"] is not None])
    out["median_centre_gap_m"] = float(np.median(gaps)) if len(gaps) else None
    labels, gt = ls.cpu().numpy(), np.asarray(fp.gt_flow, np.float64)
    diff = [float(np.linalg.norm(np.array(e["velocity"]) * objects.seconds - gt[labels == np.float32(e["label_src"])].mean(axis=0))) for e in listed]
    out["displacement_against_mean_gt_flow_m"] = dict(median=float(np.median(diff)), largest=float(np.max(diff))) if diff else None
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms of the line-of-sight check (icpflow_sight_build / _query / _segments, csrc/sight.hip) on the demo frame pair of
tests/golden/g8_demo (63 276 source x 63 322 destination points, labels of g8_demo_labels), medians of --repeat, every figure a
host clock around work that ends in a device synchronise, all in one session:

    build_ms          the depth image of the destination: fill, scatter (integer atomicMin), the 3 x 3 pass
    query_ms          one ray test of the source under the predicted flow: codes, nearest range, six counts
    segments_ms       the table per segment, both sides, with both sides' per-row codes out
    frame_sight_ms    what run_stream's `residual_sight` adds per frame pair: the image, the table, its read-back
    frame_segment_residual_ms   frame_pairs.frame_segment_residual, the call the check stands beside, in the same session
and the image's info, the twelve counts, the segments listed and their verdicts.  Not gated: nobody had measured an integer
atomicMin onto a 256 KB image on this GPU when this was written.

    python tools/dbg/sight_time.py [--repeat 30] [--origin 0 0 0] [--out profiles/sight_ms.json]
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
sys.path.insert(0, os.path.join(REPO, "tests"))
from conftest import load_golden                                              # noqa: E402
from icp_flow_amd import _lib, frame_pairs, utils_eval                        # noqa: E402


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
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    g, lab = load_golden("g8_demo"), load_golden("g8_demo_labels")
    fp = frame_pairs.FramePair(g["point_src"], g["point_dst"], lab["label_src"], lab["label_dst"], gt_flow=g["gt_flow"], name="g8_demo")
    frame_pairs.make_resident(fp, dev)
    a = frame_pairs.default_args()
    a.residual = 2.0
    registered = frame_pairs.register_frame_pair(a, fp, dev)
    ps, pd = frame_pairs._input(fp, "points_src", dev), frame_pairs._input(fp, "points_dst", dev)
    flow = registered["flow"].float().contiguous()
    labels = registered["labels_src"].float().contiguous()
    origin = tuple(ns.origin)
    _, _, _, d2b, d2a = utils_eval.segment_residual_device(ps, ps, flow, labels, pd, 2.0, per_row=True)
    image = utils_eval.sight_image(pd, origin)

    def frame_sight():
        report, look = frame_pairs.frame_segment_sight(fp, registered, dev, 2.0, origin)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seen = look()
        torch.cuda.synchronize()
        return report, seen, (time.perf_counter() - t0) * 1e3

    out = dict(points_src=len(ps), points_dst=len(pd), repeat=ns.repeat, device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO,
               origin=list(origin), params=image.params.as_dict())
    out["build_ms"] = median_ms(lambda: utils_eval.sight_image(pd, origin), ns.repeat)
    out["query_ms"] = median_ms(lambda: utils_eval.line_of_sight(image, ps, flow, near=True), ns.repeat)
    out["segments_ms"] = median_ms(lambda: utils_eval.segment_sight_device(image, ps, ps, flow, labels, d2b, d2a, per_row=True), ns.repeat)
    out["frame_sight_ms"] = float(np.median([frame_sight()[2] for _ in range(ns.repeat + 1)][1:]))
    out["frame_segment_residual_ms"] = median_ms(lambda: frame_pairs.frame_segment_residual(fp, registered, dev, 2.0), ns.repeat)
    report, seen, _ = frame_sight()
    worst = seen.annotate(report.worst(pairs=registered["pairs"]))
    out.update(image_info=dict(zip(("bad_targets", "targets_outside", "occupied_pixels"), image.info.tolist())), counts=seen.info,
               segments=len(seen), listed=len(worst), verdicts={v: sum(1 for e in worst if e["verdict"] == v) for v in utils_eval.SIGHT_VERDICTS})
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

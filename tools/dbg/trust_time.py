#!/usr/bin/env python3
"""ms of the trust byte (icpflow_flow_trust, csrc/trust.hip) on the demo frame pair of tests/golden/g8_demo (63 276 source x
63 322 destination points, labels of g8_demo_labels), medians of --repeat, every figure a host clock around work that ends in a
device synchronise, all in one session:

    call_ms             the call alone -- its two launches -- on tables and per-row arrays that are resident, with the line of sight
    call_residual_only_ms   the same without a sight table
    frame_trust_ms      frame_pairs.frame_trust with an origin: the segments' residual, the image, the segments' sight table, the
                        call, its read-back of sixteen words -- what `--residual-trust --residual-sight` adds per frame pair
    frame_trust_residual_only_ms   the same without an origin: what a bare `--save-trust` costs per frame pair
and, for either variant, the counts, the kept share and the end-point error of the kept and of the dropped rows against the
sample's gt_flow (host numpy).  Not gated: the call is new.

    python tools/dbg/trust_time.py [--repeat 30] [--origin 0 0 0] [--out profiles/trust_ms.json]
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
    pairs = registered["pairs"]
    origin = tuple(ns.origin)
    table, num, _, d2b, d2a = utils_eval.segment_residual_device(ps, ps, flow, labels, pd, 2.0, per_row=True)
    image = utils_eval.sight_image(pd, origin)
    seen, _, _, _, code = utils_eval.segment_sight_device(image, ps, ps, flow, labels, d2b, d2a, per_row=True)
    error = np.linalg.norm(np.asarray(fp.gt_flow, np.float64) - flow.cpu().numpy()[:, 0:3].astype(np.float64), axis=1)

    def judged(trust, counts):
        keep = utils_eval.trust_keep(trust).cpu().numpy()
        mean = lambda rows: float(error[rows].mean()) if rows.any() else float("nan")   # noqa: E731
        return dict(counts=counts.summary(), kept_share=counts.kept_share(), epe_all=float(error.mean()), epe_kept=mean(keep), epe_dropped=mean(~keep),
                    rows_evaluated=int(len(error)))

    out = dict(points_src=len(ps), points_dst=len(pd), segments=int(num.item()), matched_pairs=int(pairs.shape[0]), repeat=ns.repeat,
               device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO, radius=2.0, origin=list(origin),
               params=_lib.TrustParams.defaults().as_dict())
    out["call_ms"] = median_ms(lambda: utils_eval.flow_trust_device(ps, flow, labels, table, num, d2a, pairs, seen, code), ns.repeat)
    out["call_residual_only_ms"] = median_ms(lambda: utils_eval.flow_trust_device(ps, flow, labels, table, num, d2a, pairs), ns.repeat)
    out["frame_trust_ms"] = median_ms(lambda: frame_pairs.frame_trust(fp, registered, dev, 2.0, origin), ns.repeat)
    out["frame_trust_residual_only_ms"] = median_ms(lambda: frame_pairs.frame_trust(fp, registered, dev, 2.0), ns.repeat)
    out["with_line_of_sight"] = judged(*frame_pairs.frame_trust(fp, registered, dev, 2.0, origin))
    out["residual_only"] = judged(*frame_pairs.frame_trust(fp, registered, dev, 2.0))
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

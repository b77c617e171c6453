#!/usr/bin/env python3
"""ms of the residual per segment (icpflow_nn_residual_segments, csrc/segresid.hip) on the demo frame pair of
tests/golden/g8_demo (63 276 source x 63 322 destination points, labels of g8_demo_labels), r = 2.0 and r = 0.1, medians of
--repeat, every figure a host clock around work that ends in a device synchronise, both paths in one session:

    segments_ms       the new call: one grid over the destination, both sides' queries, the table per segment, the per-row
                      d2 of both sides out
    two_calls_ms      what it stands in for: two forward icpflow_nn_residual calls with per-row outputs (d2 and idx) and the
                      table of the four groups -- BEFORE (the source, no flow) and AFTER (the source plus the flow) --, each
                      building the destination's grid anew
    frame_ms          frame_pairs.frame_segment_residual: the call without per-row outputs and its one read-back
and the number of segments, how many `worst` lists, and d_info.  The expectation, unmeasured when this was written: the new
call saves about one grid build (profiles/nn_residual_ms.json: build_ms) and pays for the label order and the chunk kernels.

    python tools/dbg/segment_residual_time.py [--repeat 30] [--out profiles/segment_residual_ms.json]
"""
import argparse
import ctypes
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
    groups = frame_pairs.residual_groups(labels, registered["pairs"])
    n, m, G = len(ps), len(pd), len(utils_eval.RESIDUAL_GROUPS)
    edges = np.asarray(utils_eval.RESIDUAL_EDGES, np.float64)
    E, Lmax = len(edges), _lib.NNRS_MAX_SEGMENTS
    d2 = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    words = torch.empty(G * (E + 4) + 4, dtype=torch.int64, device=dev)
    table = torch.empty((Lmax, _lib.NNRS_COLS), dtype=torch.float64, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    info = torch.empty(6, dtype=torch.int64, device=dev)
    ws = _lib.workspace(dev, max(int(_lib._L.icpflow_nn_residual_workspace_bytes(n, m, G, E)),
                                 int(_lib._L.icpflow_nn_residual_segments_workspace_bytes(n, m, Lmax, E))))
    ed = edges.ctypes.data_as(ctypes.c_void_p)

    def one_call(f, out, radius):
        _lib.call("icpflow_nn_residual", _lib.ptr(ps), _lib.ptr(f), n, _lib.ptr(pd), m, float(radius), _lib.ptr(groups), G, ed, E, _lib.ptr(out),
                  _lib.ptr(idx), _lib.ptr(words), ctypes.c_void_p(words.data_ptr() + G * (E + 4) * 8), _lib.ptr(ws), ctypes.c_size_t(ws.numel()),
                  _lib.stream(dev))

    def two_calls(radius):
        one_call(None, d2[0], radius)
        one_call(flow, d2[1], radius)

    def segments(radius):
        _lib.call("icpflow_nn_residual_segments", _lib.ptr(ps), _lib.ptr(ps), _lib.ptr(flow), _lib.ptr(labels), n, _lib.ptr(pd), m, float(radius),
                  ed, E, _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(d2[0]), _lib.ptr(d2[1]), _lib.ptr(info), _lib.ptr(ws),
                  ctypes.c_size_t(ws.numel()), _lib.stream(dev))

    out = dict(points_src=n, points_dst=m, repeat=ns.repeat, device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO,
               matched_cluster_pairs=int(registered["pairs"].shape[0]), radii={})
    for radius in (2.0, 0.1):
        two = median_ms(lambda: two_calls(radius), ns.repeat)
        rows_two = [t.clone() for t in d2]
        one = median_ms(lambda: segments(radius), ns.repeat)
        same = all(torch.equal(x, y) for x, y in zip(rows_two, d2))          # the same per-row bits from either path
        frame = median_ms(lambda: frame_pairs.frame_segment_residual(fp, registered, dev, radius), ns.repeat)
        report = frame_pairs.frame_segment_residual(fp, registered, dev, radius)
        out["radii"][f"{radius:g}"] = dict(segments_ms=one, two_calls_ms=two, saved_ms=two - one, frame_ms=frame, per_row_bits_equal=bool(same),
                                           segments=len(report), listed=len(report.worst(pairs=registered["pairs"])), info=report.info)
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

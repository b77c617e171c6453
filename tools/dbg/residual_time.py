#!/usr/bin/env python3
"""ms of the nearest-neighbour residual (icpflow_nn_residual, csrc/nnresid.hip) on the demo frame pair of tests/golden/g8_demo
(63 276 source x 63 322 destination points, labels of g8_demo_labels), r = 2.0 and r = 0.1, medians of --repeat, every figure
a host clock around work that ends in a device synchronise:

    build_ms          the call with n = 0 queries: the grid over the destination cloud alone (count, scan, scatter)
    query_ms          the call with d2 and idx out and no table, minus build_ms (a difference of two medians)
    table_ms          the call with the table as well, minus the call without it
    frame_ms          one whole run_stream residual: frame_pairs.frame_residual, the four calls and their read-back, on the
                      flow the registration of this frame pair gives
    nn_batch_ms       beside them utils_helper.nearest_neighbor_batch (icpflow_nn_batch, B = 1), the all-pairs scan, on the same
                      clouds -- or the reason it refused the size
and d_info's occupied buckets and longest bucket of the destination's grid.  The product's query is the binned form; the first
form, a lane per query, is a variant build of the same sources, timed by the same tool:

    python tools/dbg/residual_time.py [--repeat 30] [--out FILE.json]
    python icp_flow_amd/build.py --define ICPFLOW_NNR_LANE_QUERY --out tools/dbg/libicpflow_lane_query.so
    ICPFLOW_HIP_LIB=tools/dbg/libicpflow_lane_query.so python tools/dbg/residual_time.py --form "lane per query" [--out FILE.json]
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
from icp_flow_amd import _lib, frame_pairs, utils_eval, utils_helper          # noqa: E402


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
    ap.add_argument("--form", default="binned", help="the query form of the library that is loaded (a label for the output)")
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
    groups = frame_pairs.residual_groups(registered["labels_src"].float(), registered["pairs"])
    n, m, G = len(ps), len(pd), len(utils_eval.RESIDUAL_GROUPS)
    edges = np.asarray(utils_eval.RESIDUAL_EDGES, np.float64)
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    words = torch.empty(G * (len(edges) + 4) + 4, dtype=torch.int64, device=dev)
    info = ctypes.c_void_p(words.data_ptr() + G * (len(edges) + 4) * 8)
    ws = _lib.workspace(dev, int(_lib._L.icpflow_nn_residual_workspace_bytes(n, m, G, len(edges))))

    def call(rows, radius, per_row, table):
        _lib.call("icpflow_nn_residual", _lib.ptr(ps), _lib.ptr(flow), rows, _lib.ptr(pd), m, float(radius), _lib.ptr(groups), G,
                  edges.ctypes.data_as(ctypes.c_void_p), len(edges), _lib.ptr(d2) if per_row else None, _lib.ptr(idx),
                  _lib.ptr(words) if table else None, info, _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(dev))

    out = dict(points_src=n, points_dst=m, repeat=ns.repeat, device=torch.cuda.get_device_name(dev), query_form=ns.form, library=_lib.BUILD_INFO,
               matched_cluster_pairs=int(registered["pairs"].shape[0]), radii={})
    for radius in (2.0, 0.1):
        build = median_ms(lambda: call(0, radius, False, False), ns.repeat)
        rows = median_ms(lambda: call(n, radius, True, False), ns.repeat)
        full = median_ms(lambda: call(n, radius, True, True), ns.repeat)
        host = words.cpu().numpy()
        table = utils_eval.ResidualTable.from_words(host[:-4], G, utils_eval.RESIDUAL_EDGES, radius)
        frame = median_ms(lambda: frame_pairs.frame_residual(fp, registered, dev, radius), ns.repeat)
        after, _, before, _ = frame_pairs.frame_residual(fp, registered, dev, radius)
        out["radii"][f"{radius:g}"] = dict(build_ms=build, query_ms=rows - build, table_ms=full - rows, call_ms=full, frame_ms=frame,
                                           occupied_buckets=int(host[-2]), longest_bucket=int(host[-1]), hit_rate=table.hit_rate(),
                                           mean_before=before.mean(), mean_after=after.mean(), mean_matched_before=before.mean(3),
                                           mean_matched_after=after.mean(3))
    try:
        q4, t4 = ps[None].contiguous(), pd[None].contiguous()
        out["nn_batch_ms"] = median_ms(lambda: utils_helper.nearest_neighbor_batch(q4, t4), ns.repeat)
    except RuntimeError as e:            # (the all-pairs scan is shaped for cluster pairs: it may refuse a whole frame)
        out["nn_batch_ms"] = None
        out["nn_batch_refused"] = str(e)
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

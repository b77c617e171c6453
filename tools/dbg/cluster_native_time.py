"""Developer tool: ms per UNLABELLED demo frame pair (clustering + registration + flow, inputs resident) through the Python
clustering and through the native call (icpflow_track_frame_points), for both clusterers, one at a time and four in flight.

    python tools/dbg/cluster_native_time.py [--rounds 5] [--ways python,native] [--out FILE]

The ways are timed in alternating rounds inside one process; the figure of a way is the median of its rounds.  One at a time:
`register_frame_pair_native` with a device synchronise behind every frame pair.  In flight: 16 frame pairs through
`register_in_flight_native` (four host threads, a stream each), wall time over 16.  A tree without the native call (an older
checkout) runs --ways python: `native_cluster` is an attribute it never reads.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from conftest import load_golden  # noqa: E402
from icp_flow_amd import frame_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ways", default="python,native")
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    g = load_golden("g8_demo")
    fps = [frame_pairs.make_resident(frame_pairs.FramePair(g["point_src"], g["point_dst"], None, None, None, g["gt_flow"]), dev)
           for _ in range(16)]
    ways = ns.ways.split(",")

    def args(cluster, way):
        a = frame_pairs.default_args(max_points=10000, cluster=cluster, epsilon=0.25, min_cluster_size=20, num_clusters=200)
        if way == "native":
            a.native_cluster = True
        return a

    def alone(a, reps):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = frame_pairs.register_frame_pair_native(a, fps[0], dev)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
            assert frame_pairs._served(out)
        return float(np.median(ts))

    def in_flight(a):
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = sum(1 for _ in frame_pairs.register_in_flight_native(a, fps, dev, in_flight=4))
        torch.cuda.synchronize()
        assert n == len(fps)
        return (time.perf_counter() - t) * 1e3 / n

    res = {}
    for cluster, reps in (("dbscan", 30), ("hdbscan", 12)):
        cfg = {w: args(cluster, w) for w in ways}
        for a in cfg.values():        # warm every path: code objects, workspaces, worker threads
            alone(a, 3)
            in_flight(a)
        rounds = {(w, k): [] for w in ways for k in ("alone", "in_flight_4")}
        for _ in range(ns.rounds):
            for w in ways:
                rounds[(w, "alone")].append(alone(cfg[w], reps))
                rounds[(w, "in_flight_4")].append(in_flight(cfg[w]))
        res[cluster] = {f"{w}_{k}": {"ms_per_frame_pair": round(float(np.median(v)), 3), "rounds": [round(x, 3) for x in v]}
                        for (w, k), v in rounds.items()}
    line = json.dumps({"tool": "cluster_native_time", "frame_pair": "demo, 126598 points, unlabelled, max_points 10000",
                       "device": torch.cuda.get_device_name(0), **res})
    print(line)
    if ns.out:
        with open(ns.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""ms per frame of icpflow_ground_segment (csrc/ground.hip): a 120 000-point synthetic frame (tests/ground_scenes.py) and, when
the golden files are there, the demo frame's source cloud (tests/golden/g8_demo*.npz).  HIP events around one call on a
resident cloud with a preallocated workspace, 5 warm-up calls, the median of 20.

    python tools/dbg/ground_time.py [--repeat 20] [--out FILE.json]
"""
import argparse
import ctypes
import glob
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from icp_flow_amd import _lib   # noqa: E402


def time_cloud(pts, repeat, dev):
    x = torch.from_numpy(np.ascontiguousarray(pts[:, 0:3].astype(np.float32))).to(dev)
    n = len(x)
    par = _lib.GroundParams.defaults()
    need = int(_lib._L.icpflow_ground_workspace_bytes(n, ctypes.byref(par)))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    labels = torch.empty(n, dtype=torch.uint8, device=dev)
    table = torch.empty((_lib.GROUND_PATCHES, _lib.GROUND_TABLE_COLS), dtype=torch.float64, device=dev)
    go = lambda: _lib.call("icpflow_ground_segment", _lib.ptr(x), 3, n, ctypes.byref(par), _lib.ptr(labels), _lib.ptr(table),   # noqa: E731
                           _lib.ptr(ws), ctypes.c_size_t(need), _lib.stream(dev))
    for _ in range(5):
        go()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        go()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t = table.cpu().numpy()
    return dict(points=n, ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                nonground=int(labels.sum()), patches_of_10=int((t[:, 0] >= 10).sum()), largest_patch=int(t[:, 0].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    import ground_scenes
    out = {"synthetic_120000": time_cloud(ground_scenes.frame()[0], ns.repeat, dev)}
    for path in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "g8_demo*.npz"))):
        z = np.load(path)
        key = next((k for k in ("point_src", "points_src") if k in z.files), None)
        if key is not None and z[key].ndim == 2 and z[key].shape[1] >= 3:
            out[os.path.basename(path) + ":" + key] = time_cloud(z[key], ns.repeat, dev)
            break
    print(json.dumps(out))
    if ns.out:
        with open(ns.out, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()

"""ms per frame of the ego-motion estimate at the demo frame's size, split into down-sampling, registration and map update
(HIP events around the pieces of the C ABI, which is what icpflow_ego_register_frame chains) and the deskew launch of a
stamped frame, next to the whole call and to the fp64 restatement's CPU time for the same frames.

    python tools/dbg/ego_motion_time.py [--frames 32] [--warmup 4]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--restatement-frames", type=int, default=5)
    ns = ap.parse_args()
    import ego_motion_restatement as rest
    import ego_motion_scenes as scenes
    from icp_flow_amd import utils_ego_motion
    frames, truth = scenes.exact_path(num_frames=ns.frames + 1, step=scenes.rigid(0.4, 0.0, 0.2))
    dev = torch.device("cuda:0")
    resident = [torch.from_numpy(f).to(dev) for f in frames]
    ego = utils_ego_motion.egomotion(None, dev, max_points=max(len(f) for f in frames), map_capacity=1 << 16)
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    # (a) the whole call, frame after frame
    for _ in range(max(ns.warmup // 4, 1)):
        ego.reset()
        for f in resident[: 4]:
            ego.register_frame(f, None)
    ego.reset()
    whole, iters = [], []
    for f in resident:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ego.register_frame(f, None)
        whole.append((time.perf_counter() - t0) * 1e3)
        iters.append(ego.frame_info()["iterations"])
    poses = ego.poses
    info = ego.frame_info()
    # (b) the pieces, teacher-forced with the poses of (a)
    ego.reset()
    split = dict(downsample=[], registration=[], map_update=[], step_iterations=[])
    for j, f in enumerate(resident):
        e = [ev() for _ in range(4)]
        idx_ds, idx_source = ego.downsample(f)
        src, ds = f[idx_source].contiguous(), f[idx_ds].contiguous()
        torch.cuda.synchronize()
        e[1].record()
        # (the guess of a first frame pair: the previous pose, under the initial threshold -- the longest loop a frame sees)
        res = ego.register_step(src, poses[j - 1] if j else np.eye(4), 10.0)
        e[2].record()
        ego.map_add(ds, poses[j])
        e[3].record()
        torch.cuda.synchronize()
        if j >= 1:
            split["registration"].append(e[1].elapsed_time(e[2]))
            split["map_update"].append(e[2].elapsed_time(e[3]))
            split["step_iterations"].append(int(res.cpu()[16]))
    # the down-sampling alone (its call ends in a read-back of the two counts: timed with events around the enqueue)
    for f in resident[1:]:
        a, b = ev(), ev()
        n = len(f)
        idx = torch.empty((2, n), dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int32, device=dev)
        from icp_flow_amd import _lib
        a.record()
        _lib.call("icpflow_ego_downsample", ego._h, _lib.ptr(f), n, _lib.ptr(idx[0]), _lib.ptr(idx[1]), _lib.ptr(counts), _lib.stream(dev))
        b.record()
        torch.cuda.synchronize()
        split["downsample"].append(a.elapsed_time(b))
    # the deskew launch alone (step 0 of a stamped frame): stamps over the sweep, the twist of the last two poses
    deskew_ms = []
    for f in resident[1:]:
        a, b = ev(), ev()
        stamps = torch.linspace(0.0, 1.0, len(f), device=dev)
        out = torch.empty((len(f), 3), dtype=torch.float32, device=dev)
        two = (ctypes.c_double * 32)(*np.stack(poses[-2:]).reshape(32))
        a.record()
        _lib.call("icpflow_egomotion_deskew", ego._h, _lib.ptr(f), _lib.ptr(stamps), len(f), two, _lib.ptr(out), _lib.stream(dev))
        b.record()
        torch.cuda.synchronize()
        deskew_ms.append(a.elapsed_time(b))
    # (c) the restatement on the CPU
    odo = rest.Odometry()
    cpu = []
    for f in frames[: ns.restatement_frames]:
        t0 = time.perf_counter()
        odo.register_frame(f, keep_map=False)
        cpu.append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))   # noqa: E731
    out = dict(points_per_frame=int(np.median([len(f) for f in frames])), last_frame=info, frames=len(whole) - 1,
               whole_call_ms=stat(whole[1 + ns.warmup:]), iterations=stat(iters[1:]),
               downsample_ms=stat(split["downsample"]), registration_ms=stat(split["registration"]), map_update_ms=stat(split["map_update"]), deskew_ms=stat(deskew_ms),
               registration_iterations=stat(split["step_iterations"]), restatement_cpu_ms=stat(cpu[1:]),
               worst_cap_m=float(max(scenes.cap_expression(p, t) for p, t in zip(poses, truth))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

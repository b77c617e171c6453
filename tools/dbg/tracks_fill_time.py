#!/usr/bin/env python3
"""ms per sample of `--tracks` with and without `--tracks-fill` (pair_judges.frame_tracks(fill=...); icpflow_object_tracks_missing
of csrc/tracks.hip,
icpflow_pairs_fill_candidates and icpflow_pairs_reregister of csrc/repair.hip) on the synthetic multi-frame sample of
tools/dbg/tracks_time.py (icp_flow_amd.synthetic.make_sequence), medians of --repeat, every figure a host clock around work that
ends in a device synchronise, all in one session:

    frame_tracks_ms             frame_tracks as `--tracks` runs it
    frame_tracks_fill_ms        ... with fill=True on the registrations as they are (the plan, its read-back, and whatever is missing)
    frame_tracks_deleted_ms     ... with one pair row of the middle gap deleted before every pass (the candidates, one registration,
                                the gap's flow, the second chain)
    fill_ms, fill_deleted_ms    of the two above, the part behind the tracks' read-back (utils_tracks.Fill.ms)
    missing_ms                  icpflow_object_tracks_missing alone over the sample's observations and segments
and what the fill found in either case.  Every pass starts from copies of the registrations (the fill replaces tensors of its
`outs`).  Not gated: the calls are new.

    python tools/dbg/tracks_fill_time.py [--repeat 20] [--out profiles/tracks_fill_ms.json]
"""
import argparse
import datetime
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from icp_flow_amd import _lib, frame_pairs, synthetic, utils_flow, utils_tracks      # noqa: E402


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
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--objects", type=int, default=40)
    ap.add_argument("--background", type=int, default=40000)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    sample = synthetic.make_sequence(seed=3, num_frames=ns.frames, n_objects=ns.objects, n_min=200, n_max=3000, speed=0.5, n_background=ns.background)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "sample.npz")
        np.savez(path, **sample)
        fps = frame_pairs.load_sequence(path, pose_source="ego_motion_gt")
    a = frame_pairs.default_args(cluster="dbscan", epsilon=0.4, min_cluster_size=10)
    a.tracks = True
    outs = [frame_pairs.register_frame_pair(a, fp, dev) for fp in fps]
    middle = len(outs) // 2
    plain = frame_pairs.frame_tracks(fps, outs, dev)
    consistent = [t for t in plain.as_list() if t["consistent"] and len(t["gaps"]) >= 3]
    pair = next((p for p, t in enumerate(plain.observation_ids[middle]) if consistent and t == consistent[0]["track"]), 0)

    def copies(delete):
        cs = [dict(out) for out in outs]
        if delete:
            fp, out = fps[middle], cs[middle]
            keep = [k for k in range(int(out["pairs"].shape[0])) if k != pair]
            out["pairs"], out["transformations"] = out["pairs"][keep].clone(), out["transformations"][keep].clone()
            src = torch.from_numpy(fp.points_src_raw if fp.points_src_raw is not None else fp.points_src).to(dev)
            out["flow"] = utils_flow.flow_estimation_torch(None, src, None, out["labels_src"], None, out["pairs"], out["transformations"],
                                                           torch.from_numpy(fp.pose).to(dev))
        return cs

    last, parts = {}, []

    def run(delete, fill):
        last["tracks"] = frame_pairs.frame_tracks(fps, copies(delete), dev, fill=fill, args=a)
        if fill:
            parts.append(last["tracks"].fill.ms)

    out = dict(rows=len(fps[0].points_dst), frames=ns.frames, gaps=len(fps), pairs=[int(o["pairs"].shape[0]) for o in outs], repeat=ns.repeat,
               device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO, date=datetime.date.today().isoformat(),
               max_residual=utils_tracks.MAX_RESIDUAL, radius=utils_tracks.FILL_RADIUS)
    out["frame_tracks_ms"] = median_ms(lambda: run(False, False), ns.repeat)
    out["frame_tracks_fill_ms"] = median_ms(lambda: run(False, True), ns.repeat)
    out["fill_ms"], out["fill_as_registered"] = float(np.median(parts[1:])), last["tracks"].fill.summary(last["tracks"])
    del parts[:]
    out["frame_tracks_deleted_ms"] = median_ms(lambda: run(True, True), ns.repeat)
    out["fill_deleted_ms"], out["fill_deleted"] = float(np.median(parts[1:])), last["tracks"].fill.summary(last["tracks"])
    state = utils_tracks.TrackState(len(fps[0].points_dst), dev)
    for fp, o in zip(fps, outs):
        rows, _, ld = frame_pairs._frame_objects_device(fp, o, dev, fp.gap * 0.1, utils_tracks.MIN_SPEED)
        state.extend(ld, rows, fp.gap, fp.gap * 0.1)
    obs = torch.cat(state.obs)
    segments, nums = torch.stack([s for s, _ in state.segments]), torch.cat([k for _, k in state.segments])
    seconds = [fp.gap * 0.1 for fp in fps]
    out["observations"], out["tracks_bound"] = int(obs.shape[0]), state.bound
    out["missing_ms"] = median_ms(lambda: utils_tracks.missing_device(obs, state.bound, segments, nums, state.gaps, seconds), ns.repeat)
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

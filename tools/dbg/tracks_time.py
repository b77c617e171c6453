#!/usr/bin/env python3
"""ms of the object tracks (icpflow_label_overlap, icpflow_object_tracks_extend, icpflow_object_tracks_fit; csrc/overlap.hip,
csrc/tracks.hip) on one synthetic multi-frame sample (icp_flow_amd.synthetic.make_sequence: --frames sweeps, --objects moving
shells over --background ground points, clustered per gap by DBSCAN), medians of --repeat, every figure a host clock around
work that ends in a device synchronise, all in one session:

    label_overlap_ms    icpflow_label_overlap alone: the shared sweep's labels of gap 1 against those of gap 2
    extend_ms           icpflow_object_tracks_extend alone: gap 2 onto the state gap 1 left (the state restored before every pass,
                        outside the clock), the gap's object rows resident
    fit_ms              icpflow_object_tracks_fit alone over the observations of all gaps, at the bound TrackState passes
    frame_tracks_ms     frame_pairs.frame_tracks: per gap two cluster tables, two box tables, the pairs' objects and the
                        extension, then the fit and the one read-back -- what `--tracks` adds per sample
and what the tracks of that sample are: the counts, the largest residual of the consistent tracks.  Not gated: the calls are new.

    python tools/dbg/tracks_time.py [--repeat 30] [--out profiles/tracks_ms.json]
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
from icp_flow_amd import _lib, frame_pairs, synthetic, utils_objects, utils_tracks      # noqa: E402


def median_ms(fn, repeat, before=None):
    times = []
    for k in range(repeat + 1):
        if before is not None:
            before()
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
    seconds = [fp.gap * utils_objects.SWEEP_SECONDS for fp in fps]
    rows = [frame_pairs._frame_objects_device(fp, out, dev, s, utils_tracks.MIN_SPEED)[0] for fp, out, s in zip(fps, outs, seconds)]
    labels = [out["labels_dst"].float().contiguous() for out in outs]
    n = len(fps[0].points_dst)

    state = utils_tracks.TrackState(n, dev)
    state.extend(labels[0], rows[0], fps[0].gap, seconds[0])
    kept = (state.track_of_row.clone(), state.next_id.clone())

    def restore():
        state.track_of_row.copy_(kept[0])
        state.next_id.copy_(kept[1])

    out = dict(rows=n, frames=ns.frames, gaps=len(fps), pairs=[int(r.shape[0]) for r in rows], repeat=ns.repeat, device=torch.cuda.get_device_name(dev),
               library=_lib.BUILD_INFO, date=datetime.date.today().isoformat(), min_iou=utils_tracks.MIN_IOU, max_residual=utils_tracks.MAX_RESIDUAL,
               min_speed=utils_tracks.MIN_SPEED, sweep_seconds=utils_objects.SWEEP_SECONDS)
    out["label_overlap_ms"] = median_ms(lambda: utils_tracks.label_overlap_device(labels[0], labels[1]), ns.repeat)
    out["extend_ms"] = median_ms(lambda: state.extend(labels[1], rows[1], fps[1].gap, seconds[1]), ns.repeat, before=restore)
    whole = utils_tracks.TrackState(n, dev)
    for lab, r, fp, s in zip(labels, rows, fps, seconds):
        whole.extend(lab, r, fp.gap, s)
    out["fit_tracks_bound"], out["fit_observations"] = whole.bound, int(sum(r.shape[0] for r in rows))
    out["fit_ms"] = median_ms(whole.fit, ns.repeat)
    out["frame_tracks_ms"] = median_ms(lambda: frame_pairs.frame_tracks(fps, outs, dev), ns.repeat)
    tracks = frame_pairs.frame_tracks(fps, outs, dev)
    out["counts"] = tracks.summary()
    listed = tracks.as_list()
    consistent = [t["residual_max"] for t in listed if t["consistent"]]
    out["largest_residual_of_consistent_tracks_m"] = max(consistent) if consistent else None
    out["segments_per_gap"] = [int(num.item()) for _, num in whole.segments]
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

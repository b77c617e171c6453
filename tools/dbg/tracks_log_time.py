#!/usr/bin/env python3
"""ms of the object tracks over a log (icpflow_rows_carry, icpflow_pair_row_ids, icpflow_object_tracks_extend_side,
icpflow_object_tracks_path; carry.hip and tracks.hip) on one synthetic log (icp_flow_amd.synthetic.make_log: --files
consecutive frame-pair files, six objects and --extra more boxes over ground at --ground-spacing, clustered per file by DBSCAN),
medians of --repeat, every figure a host clock around work that ends in a device synchronise, all in one session:

    carry_ms            icpflow_rows_carry alone: the ids of file 0's destination rows onto file 1's source rows
    pair_row_ids_ms     icpflow_pair_row_ids alone: file 1's destination rows from its pairs' ids, weights at stride 24
    extend_side_ms      icpflow_object_tracks_extend_side alone, side 0: file 1's source labels onto the carried ids (the state
                        restored before every pass, outside the clock), the file's object rows resident
    path_ms             icpflow_object_tracks_path alone over the observations of all files, at the bound the chain passes
    judge_ms_per_file   pair_judges.log_tracks over the whole log, per file: two box tables, the pairs' objects, the carry, the
                        extension and the destination ids per file, then the table and the one read-back -- what `--tracks-log` adds
    ms_per_frame_pair_without_judge   run_stream over the same files, one at a time, with no judge: the registration the judge's
                        figure stands beside (code this feature does not touch)
and what the tracks of that log are: the summary.  Not gated: the calls are new.

    python tools/dbg/tracks_log_time.py [--repeat 20] [--out profiles/tracks_log_ms.json]
"""
import argparse
import ctypes
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
from icp_flow_amd import _lib, frame_pairs, pair_judges, synthetic, utils_tracks      # noqa: E402


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
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--extra", type=int, default=34)
    ap.add_argument("--ground-spacing", type=float, default=0.24)
    ap.add_argument("--out", default=None)
    ns = ap.parse_args()
    dev = torch.device("cuda:0")
    pairs, _ = synthetic.make_log(3, ns.files, ground_spacing=ns.ground_spacing, extra=ns.extra)
    fps = [frame_pairs.FramePair(p["points_src"], p["points_dst"], pose=p["pose"], nonground_src=p["nonground_src"], nonground_dst=p["nonground_dst"],
                                 name=f"file_{k:02d}") for k, p in enumerate(pairs)]
    a = frame_pairs.default_args(**synthetic.LOG_CLUSTER)
    a.tracks_log = True
    outs = [frame_pairs.register_frame_pair(a, fp, dev) for fp in fps]
    S = synthetic.LOG_SWEEP_SECONDS
    rows = [frame_pairs._frame_objects_device(fp, out, dev, S, utils_tracks.MIN_SPEED) for fp, out in zip(fps, outs)]
    up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)    # noqa: E731

    # file 0 by hand, to have the inputs of file 1's calls resident
    first = utils_tracks.TrackState(len(fps[0].points_src), dev)
    _, _, obs0, _ = first.extend(outs[0]["labels_src"].float(), rows[0][0], 0, S, side=0)
    ids0, _ = utils_tracks.pair_row_ids_device(rows[0][2], outs[0]["pairs"], 1, obs0[:, 0].to(torch.int32), rows[0][0][:, 22])
    prev, nxt = up(fps[0].points_dst), up(fps[1].points_src)
    carried, counts = utils_tracks.rows_carry_device(prev, ids0, fps[1].pose_exact, nxt)
    kept = (carried.clone(), first.next_id.clone())
    state = utils_tracks.TrackState(len(fps[1].points_src), dev, track_of_row=carried, next_id=first.next_id, bound=first.bound)

    def restore():
        carried.copy_(kept[0])
        first.next_id.copy_(kept[1])

    ls1, ld1 = outs[1]["labels_src"].float().contiguous(), rows[1][2]
    _, _, obs1, _ = state.extend(ls1, rows[1][0], 0, S, side=0)
    pid1 = obs1[:, 0].to(torch.int32)

    out = dict(rows_per_sweep=[len(fp.points_src) for fp in fps], files=ns.files, pairs=[int(r[0].shape[0]) for r in rows], repeat=ns.repeat,
               device=torch.cuda.get_device_name(dev), library=_lib.BUILD_INFO, date=datetime.date.today().isoformat(),
               radius=utils_tracks.CARRY_RADIUS, min_share=utils_tracks.CARRY_MIN_SHARE, max_dv=utils_tracks.MAX_DV, min_speed=utils_tracks.MIN_SPEED,
               sweep_seconds=S, carry_counts_file_1=[int(v) for v in counts.cpu().numpy()])
    out["carry_ms"] = median_ms(lambda: utils_tracks.rows_carry_device(prev, ids0, fps[1].pose_exact, nxt), ns.repeat)
    out["pair_row_ids_ms"] = median_ms(lambda: utils_tracks.pair_row_ids_device(ld1, outs[1]["pairs"], 1, pid1, rows[1][0][:, 22]), ns.repeat)
    out["extend_side_ms"] = median_ms(lambda: state.extend(ls1, rows[1][0], 0, S, side=0), ns.repeat, before=restore)
    chain = pair_judges.LogChain(dev, S)
    for fp, o in zip(fps, outs):
        chain.add(fp, o)
    out["path_tracks_bound"], out["path_observations"] = chain.bound, int(sum(o.shape[0] for o in chain.obs))
    every = torch.cat(chain.obs)
    step = up(np.repeat(np.arange(ns.files, dtype=np.int32), [int(o.shape[0]) for o in chain.obs]))
    frames = up(pair_judges.log_frames(chain.poses))
    paths = torch.empty((chain.bound, _lib.TRACK_PATH_COLS), dtype=torch.float64, device=dev)
    path_counts = torch.empty(_lib.TRACK_PATH_COUNTS, dtype=torch.int64, device=dev)
    out["path_ms"] = median_ms(lambda: _lib.call("icpflow_object_tracks_path", _lib.ptr(every), _lib.ptr(step), int(every.shape[0]), _lib.ptr(frames),
                                                 ns.files, chain.bound, ctypes.byref(chain.params), _lib.ptr(paths), _lib.ptr(path_counts),
                                                 _lib.stream(dev)), ns.repeat)
    out["judge_ms_per_file"] = median_ms(lambda: pair_judges.log_tracks(fps, outs, dev, S), ns.repeat) / ns.files
    plain = frame_pairs.default_args(**synthetic.LOG_CLUSTER)
    frame_pairs.run_stream(plain, fps, dev)                       # (a first pass: page-in, allocator)
    out["ms_per_frame_pair_without_judge"] = float(np.median([frame_pairs.run_stream(plain, fps, dev)["ms_per_frame_pair"] for _ in range(3)]))
    out["counts"] = pair_judges.log_tracks(fps, outs, dev, S).summary()
    print(json.dumps(out))
    if ns.out:
        os.makedirs(os.path.dirname(os.path.abspath(ns.out)), exist_ok=True)
        with open(ns.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

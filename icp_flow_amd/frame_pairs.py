"""Frame-pair stream: the unit of work above the registration path.

A frame pair is what the reference's loop hands to `track` (main.py:184-215, demo.py:37-71): two
ego-compensated, ground-free clouds with precomputed cluster labels (ground -1e8, noise -1,
clusters >= 0), the relative ego pose and -- for evaluation -- the ground-truth flow of the source
points.  On disk: one .npz per pair with keys

    points_src [Ns,3]  points_dst [Nd,3]  labels_src [Ns]  labels_dst [Nd]
    pose [4,4] (optional, identity)       gt_flow [Ns,3] (optional)     mask [Ns] (optional)

or the reference's Argoverse/demo keys (dataset_argo.py:34-45: pc1, pc2, pc1_flows_valid_idx,
pc2_flows_valid_idx, gt_flow_0_1) plus labels_src / labels_dst (clustering is precomputed in the BASELINE
configs).  A pair WITHOUT labels is clustered on the GPU when the arguments say how (`cluster="hdbscan"`
-- what the reference's scripts select, --if_hdbscan -- or `cluster="dbscan"`, with min_cluster_size /
num_clusters (/ epsilon): both clouds stacked dst-first and clustered jointly as demo.py:210 /
dataset_argo.py:119 do, utils_cluster.cluster_pcd; optional keys nonground_src /
nonground_dst mark the rows to cluster).

A Waymo / nuScenes sample of the reference (dataset_pca.py:41-45: one npz per SEQUENCE with raw_points,
time_indice, ..., and the ego poses under `ego_motion` -- the reference's <split>_pose files -- or
`ego_motion_gt`) is a multi-gap sample: `load_sequence` turns it into the num_frames - 1 frame pairs
(frame j -> frame 0, j = 1 .. num_frames - 1) the reference's loop registers (dataset_pca.py:164-198,
main.py:189-200): source = frame j moved by its ego pose, destination = frame 0, translation_frame =
2 * max(speed * j, |ego translation of frame j|), flow on the RAW source points with the ego pose composed
in (main.py:230-234, utils_flow.py:23-50).  Ground segmentation is upstream (BASELINE: "precomputed"): a
`nonground` key [m] marks the rows to cluster; without it every point is clustered.

`run_stream` registers every pair of a directory (round-robin over ranks: frame pairs are
independent, main.py:184), and reports ms / frame pair and the reference's accuracy metrics.

    python -m icp_flow_amd.frame_pairs DIR [--max-points 10000] [--speed 1.0] [--repeat 3]

`--residual [R]` judges every frame pair WITHOUT ground truth as well: the nearest-neighbour residual of the warped source
against the destination, truncated at R metres (2.0 when given bare), before and after the registration, both directions
(`pair_judges.frame_residual`, icpflow_nn_residual); the summary gains a `residual` block and `ms_residual_per_frame_pair`.

    python -m icp_flow_amd.frame_pairs DIR --residual [R] [--in-flight 4]

`--residual-segments [FILE]` lists the segments (clusters) that still fit badly under the flow, and `--residual-sight [X Y Z]`
says of each whether the destination sweep contradicts it ("seen through") or merely lost it ("lost from view":
`pair_judges.frame_segment_sight`, icpflow_sight_*); the summary gains `residual_sight` and `ms_sight_per_frame_pair`.

This module holds the loaders of sequences and samples, the registration paths, the two in-flight schedulers, both drivers
(`run_stream`, `run_sequences`) and the command line.  The `FramePair` class, its file and its device copies are pair_data.py's,
the judges of a registered frame pair (the `frame_*` device functions, the `residual_*` helpers and the six classes run_stream
calls) pair_judges.py's; their names are imported here, so `frame_pairs.FramePair`, `frame_pairs.frame_trust` & co. stay.

`run_sequences` (`--protocol reference`) evaluates whole sequence files by the reference's metric protocol instead
(utils_eval.py:185-368, main.py:173-181, 285-296): the frame pairs of a file as above, their flows assembled on the device
into the sequence's flow (zeros for frame 0, main.py:217-260), one pass of icpflow_seq_metrics over it and ONE small
read-back per sequence -- the table from which the reference's 6 x (num_frames + 1) meters are updated.  A sample without a
`scene_flow` key (every sample of the reference) gets its ground truth from `inst_labels`, `bbox_tsfm` and `ego_motion_gt`
on the GPU (dataset_pca.py:66-69, utils_loading.py).

    python -m icp_flow_amd.frame_pairs DIR --protocol reference --num-frames 5 --range-x 32 --range-y 32 [--eval-ground]
                                           [--range-z 0.0 --ground-slack 0.3] [--ground patchwork]
                                           [--if-verbose] [--report worst.json [--report-epe 2.0]]

`--dataset argo` evaluates Argoverse 2 files (pc1, pc2, pc*_flows_valid_idx, gt_flow_0_1, pc1_classes; dataset_argo.py:34-101)
the same way, one two-frame sample per file: the sample and its static / dynamic and foreground / background labels are built
on the device (`load_argo_sample`, icpflow_seq_argo_sample).  main.sh:38's ranges:

    python -m icp_flow_amd.frame_pairs DIR --protocol reference --dataset argo --range-x 10000 --range-y 10000
                                           --range-z -10000 --ground-slack 0 --cluster hdbscan --speed 1.67

`--class-table meta|fine` (with `--dataset argo`) prints, after the reference's table, one line per meta category (fine: and per
category) and speed bucket -- n, EPE, mean speed, the shares of the error splits -- and the three-way EPE, from one more pass
(icpflow_seq_class_table) and one more small read-back; `--save-flows` writes every sequence's flow and poses next to its
split (`flow_file`: <split>_icp_flow[_ego], main.py:265-284), `--save-metrics FILE` the reference's closing file
(main.py:298-312).  Under more than one process the files are dealt round-robin, every rank keeps one record per file, and
one all_gather and a replay in file order (`merge_sequence_records`) give every rank the single process's table bit for bit.

`--bucketed-epe` (with `--dataset argo`, independent of `--class-table`) prints the bucket-normalised EPE of the Argoverse 2
2024 challenge: per class a static EPE and a speed-normalised dynamic EPE over 51 speed buckets, and their means, from one more
pass (icpflow_seq_bucket_table) and one more small read-back; the table rides the same records under more than one process.
The challenge evaluates the 70 m x 70 m box, `--range-x 35 --range-y 35`.

`--if-verbose` is the reference's verbose loop (utils_debug.debug_frame, utils_flow.flow_evaluation): per frame pair three
lines (overall, static, dynamic) and the per-segment evaluation, from one more pass over what is resident
(icpflow_seq_segment_table) and a read-back of two small tables.
"""
import argparse
import glob
import json
import os
import queue
import threading
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import utils_eval, utils_flow, utils_objects, utils_track, utils_tracks
# the frame pair itself and the judges of a registered one live in modules of their own; their names stay reachable here
from .pair_data import FramePair, _input, _upload, load_frame_pair, make_resident, save_frame_pair  # noqa: F401
from .pair_judges import (RESIDUAL_SEGMENTS_SHOWN, LogTrackJudge, ObjectJudge, ResidualJudge, SegmentJudge, SightJudge, TrackJudge, TrustJudge,  # noqa: F401
                          _frame_objects_device, _residual_flat, _residual_unflat, _residual_zero, _source_labels, frame_objects,
                          frame_residual, frame_segment_residual, frame_segment_sight, frame_tracks, frame_trust, residual_block,
                          residual_groups, residual_tables)

# demo.sh:9-13 / main.sh flags of the registration stage
DEFAULT_ARGS = dict(max_points=10000, min_cluster_size=20, translation_frame=2.0, thres_dist=0.1, thres_box=0.1,
                    thres_rot=0.1, thres_error=0.2, thres_iou=0.2, chunk_size=50, speed=None,
                    cluster=None, epsilon=0.25, num_clusters=200, range_x=None, range_y=None,
                    # not a flag of the reference: candidate batches padded to the longest cluster of the stage instead of
                    # max_points (utils_match._stage_rows; False = the reference's width, same registrations)
                    tight_padding=True,
                    # not a flag of the reference: one call into the library per frame pair (icpflow_track_frame, the host half of
                    # match_pcds in C++, a host thread per frame pair in flight); False = the Python host (generators), same bits
                    native_host=True)


def default_args(**over):
    d = dict(DEFAULT_ARGS)
    d.update(over)
    return SimpleNamespace(**d)


def is_sequence(path):
    with np.load(path) as z:
        return "raw_points" in z.files and "time_indice" in z.files


def _pose_file(path):
    """The reference keeps estimated ego poses next to the split: .../val/x.npz -> .../val_pose/x.npz, key
    `ego_motion` (dataset_pca.py:118-125).  Only a DIRECTORY COMPONENT named train / val / test is a split (the last one
    wins): '/latest/val/x.npz' -> '/latest/val_pose/x.npz', never '/latest_pose/...'."""
    parts = os.path.normpath(path).split(os.sep)
    for k in range(len(parts) - 2, -1, -1):
        if parts[k] in ("train", "val", "test"):
            cand = os.sep.join(parts[:k] + [parts[k] + "_pose"] + parts[k + 1:])
            return cand if os.path.isfile(cand) else None
    return None


def _estimate_poses(path, raw, t, args, point_time=None):
    """pose_source="estimate": the ego poses of the sample's frames from its raw points (every point of a frame, before any
    crop of the scene: the reference estimates on the whole sweep, dataset_pca.py:126-130).  `point_time` [m], the file's
    optional per-point stamps (in [0, 1] over each sweep), is used only when args.ego_motion turns deskewing on."""
    from . import utils_ego_motion
    if len(t) == 0 or t.min() < 0:
        raise ValueError(f"{path}: time_indice does not describe a sequence")
    frames = [raw[t == j].astype(np.float32) for j in range(int(t.max()) + 1)]
    stamps = None
    if point_time is not None and utils_ego_motion.read_motion(args)["deskew"]:
        if point_time.shape != t.shape:
            raise ValueError(f"{path}: point_time {point_time.shape} does not go with time_indice {t.shape}")
        stamps = [point_time[t == j].astype(np.float32) for j in range(len(frames))]
    poses = utils_ego_motion.estimate_poses(frames, args, getattr(args, "ego_device", None) if args is not None else None,
                                            timestamps=stamps)
    if args is not None and getattr(args, "save_poses", False):
        parts = os.path.normpath(os.path.abspath(path)).split(os.sep)
        for k in range(len(parts) - 2, -1, -1):
            if parts[k] in ("train", "val", "test"):
                side = os.sep.join(parts[:k] + [parts[k] + "_pose"] + parts[k + 1:])
                os.makedirs(os.path.dirname(side), exist_ok=True)
                np.savez(side, ego_motion=poses)
                break
        else:
            raise ValueError(f"{path}: save_poses needs a split directory (train / val / test) to put <split>_pose next to")
    return poses


POSE_SOURCES = ("auto", "pose_file", "ego_motion", "ego_motion_gt", "estimate")


def load_sequence(path, args=None, pose_source=None):
    """A multi-frame sample in the reference's Waymo / nuScenes format (dataset_pca.py:41-45) -> the list of
    frame pairs of the reference's loop, gap j = 1 .. num_frames - 1 (dataset_pca.py:164-198).
    Keys: raw_points [m,>=3], time_indice [m] (0 .. F-1), ego poses [F,4,4]; optional nonground [m] (ground segmentation
    is upstream), scene_flow [m,3] (ground truth, dataset_pca.py:67-69), labels [m] (precomputed per-frame cluster
    labels are NOT possible in this format: frames are clustered jointly per gap).  args.range_x / range_y crop
    the scene like dataset_pca.py:61-64.

    Ego poses (`pose_source`, default args.pose_source or "auto"): the reference reads ESTIMATED poses from its
    <split>_pose files (key `ego_motion`, dataset_pca.py:118-125) and estimates them itself (KISS-ICP, dataset_pca.py:126-135)
    when the file is missing.  "pose_file": that file, an error without it; "ego_motion": the key of that name in the
    sample itself; "ego_motion_gt": the GROUND-TRUTH poses of the sample -- accuracy measured with them is not the
    reference's protocol; "auto": pose file, else in-file `ego_motion`, else `ego_motion_gt` WITH a warning;
    "estimate" (explicit only, "auto" never picks it; needs a GPU): the poses are estimated from the sample's raw points,
    frame by frame, by utils_ego_motion (scan-to-map odometry on the GPU; constants: args.ego_config; args.ego_motion =
    dict(deskew=True) deskews every frame by the file's optional `point_time` [m], stamps in [0, 1] over each sweep), and written to the
    <split>_pose file only when args.save_poses is set (as the reference does, dataset_pca.py:131-135).  Every
    frame pair records where its pose came from (`FramePair.pose_source`, carried into run_stream's results)."""
    import warnings
    source = pose_source or (getattr(args, "pose_source", None) if args is not None else None) or "auto"
    if source not in POSE_SOURCES:
        raise ValueError(f"pose_source must be one of {POSE_SOURCES} (got {source!r})")
    with np.load(path) as z:
        keys = set(z.files)
        raw = np.asarray(z["raw_points"])[:, 0:3].astype(np.float64)
        t = np.asarray(z["time_indice"]).astype(np.int64)
        side = _pose_file(path) if source in ("auto", "pose_file") else None
        if side is not None:
            with np.load(side) as zp:
                poses = np.asarray(zp["ego_motion"]).astype(np.float64)
            used = "pose_file"
        elif source == "estimate":
            poses, used = _estimate_poses(path, raw, t, args, np.asarray(z["point_time"]) if "point_time" in keys else None), "estimate"
        elif source == "pose_file":
            raise FileNotFoundError(f"{path}: no <split>_pose file next to the split directory (pose_source='pose_file')")
        elif source in ("auto", "ego_motion") and "ego_motion" in keys:
            poses, used = np.asarray(z["ego_motion"]).astype(np.float64), "ego_motion"
        elif source in ("auto", "ego_motion_gt") and "ego_motion_gt" in keys:
            poses, used = np.asarray(z["ego_motion_gt"]).astype(np.float64), "ego_motion_gt"
            if source == "auto":
                warnings.warn(f"{path}: no estimated ego poses (no <split>_pose file, no `ego_motion` key): falling back to "
                              "GROUND-TRUTH poses `ego_motion_gt`; the reference would estimate them (dataset_pca.py:126-130). "
                              "Pass pose_source='ego_motion_gt' to accept this silently.", stacklevel=2)
        else:
            raise KeyError(f"{path}: no ego poses for pose_source={source!r} (keys: {sorted(keys)})")
        nonground = np.asarray(z["nonground"]).astype(bool) if "nonground" in keys else None
        gt = np.asarray(z["scene_flow"])[:, 0:3].astype(np.float32) if "scene_flow" in keys else None
    if raw.shape[0] != t.shape[0] or poses.shape[1:] != (4, 4) or poses.shape[0] != t.max() + 1:
        raise ValueError(f"{path}: raw_points / time_indice / ego poses do not describe one sequence")
    rx, ry = (getattr(args, "range_x", None), getattr(args, "range_y", None)) if args is not None else (None, None)
    if rx is not None and ry is not None:
        keep = (np.abs(raw[:, 0]) < rx) & (np.abs(raw[:, 1]) < ry)                  # dataset_pca.py:61-64
        raw, t = raw[keep], t[keep]
        nonground = None if nonground is None else nonground[keep]
        gt = None if gt is None else gt[keep]
    out = []
    dst = raw[t == 0]
    for j in range(1, poses.shape[0]):
        m = t == j
        src_raw = raw[m]
        hom = np.concatenate([src_raw, np.ones((len(src_raw), 1))], axis=1)
        src_ego = (hom @ poses[j].T)[:, 0:3]                                          # utils_helper.py:89-93
        out.append(FramePair(src_ego, dst, None, None, poses[j], None if gt is None else gt[m], None,
                             name=f"{os.path.basename(path)}#gap{j}",
                             nonground_src=None if nonground is None else nonground[m],
                             nonground_dst=None if nonground is None else nonground[t == 0],
                             gap=j, points_src_raw=src_raw, pose_source=used, sequence=path))
    return out


def load_any(path, args=None, pose_source=None):
    """-> list of FramePair: one for a frame-pair file, num_frames - 1 for a sequence file."""
    return load_sequence(path, args, pose_source) if is_sequence(path) else [load_frame_pair(path)]


def list_frame_pairs(directory):
    return sorted(glob.glob(os.path.join(directory, "**", "*.npz"), recursive=True))


def shard_round_robin(items, rank, world):
    """frame pairs are dealt round-robin to ranks (keeps the association of a frame
    pair on one GPU)."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world of {world}")
    return list(items[rank::world])


def frame_translation(args, pose, gap=1):
    """main.py:200: translation_frame = 2 * max(speed * gap, |ego translation|); unchanged when the
    caller fixed translation_frame (speed None), as demo.py:205 does."""
    if getattr(args, "speed", None) is None:
        return float(args.translation_frame)
    return float(max(args.speed * gap, float(np.linalg.norm(np.asarray(pose)[0:3, 3])))) * 2.0


def cluster_frame_pair(args, ps, pd, nonground_src=None, nonground_dst=None):
    """Joint clustering of a frame pair as demo.py:210 / dataset_argo.py:112-121 do it: both clouds stacked
    dst-first, one cluster_pcd call, labels split back.  -> (labels_src, labels_dst) float32 device tensors."""
    if getattr(args, "cluster", None) not in ("dbscan", "hdbscan"):
        raise ValueError("frame pair without cluster labels: pass precomputed labels_src / labels_dst or set "
                         "args.cluster = 'hdbscan' | 'dbscan'")
    from . import utils_cluster
    dev = ps.device
    ones = lambda n: torch.ones(n, dtype=torch.bool, device=dev)
    m_src = ones(len(ps)) if nonground_src is None else torch.as_tensor(nonground_src, device=dev).bool()
    m_dst = ones(len(pd)) if nonground_dst is None else torch.as_tensor(nonground_dst, device=dev).bool()
    a = SimpleNamespace(epsilon=float(args.epsilon), min_cluster_size=int(args.min_cluster_size),
                        num_clusters=int(args.num_clusters), if_hdbscan=args.cluster == "hdbscan")
    if getattr(args, "native_cluster", False):     # icpflow_cluster_pcd: both segments as they are, no stack, no numpy
        l_dst, l_src = utils_cluster.cluster_pcd_native(a, pd, ps, None if nonground_dst is None else m_dst,
                                                        None if nonground_src is None else m_src)
        return l_src, l_dst
    labels = utils_cluster.cluster_pcd(a, torch.cat([pd, ps], dim=0), torch.cat([m_dst, m_src], dim=0)).float()
    return labels[len(pd):].contiguous(), labels[: len(pd)].contiguous()


_stream_pool = {}


def register_frame_pair_steps(args, fp, device, gap=None, asynchronous=False):
    """One frame pair through (cluster_pcd when it carries no labels +) track() + flow_estimation_torch() on `device`, as
    a generator that yields at every device -> host hand-over of the association (utils_match.match_pcds_steps) and
    returns dict(pairs [P,10], transformations [P,4,4], flow [Ns,3]) of device tensors."""
    from . import utils_match
    a = SimpleNamespace(**vars(args))
    a.translation_frame = frame_translation(args, fp.pose_exact, fp.gap if gap is None else gap)
    device = torch.device(device)
    ps = _upload(fp.points_src, device)
    pd = _upload(fp.points_dst, device)
    if fp.labels_src is None:
        ls, ld = cluster_frame_pair(args, ps, pd, fp.nonground_src, fp.nonground_dst)
    else:
        ls = _upload(fp.labels_src, device)
        ld = _upload(fp.labels_dst, device)
    pose = torch.from_numpy(fp.pose).to(device)
    # main.py:139 seeds torch's global generator once; a private generator with the same seed gives the same
    # draws (random subsampling of over-long clusters) without touching the caller's global RNG state
    a.generator = torch.Generator()
    a.generator.manual_seed(0)
    # multi-gap sample: flow of the RAW source points, the ego pose composed in (main.py:230-234; T registers the
    # ego-compensated cloud, so a point moves by T * pose); frame-pair files hand over ego-compensated clouds, their `pose`
    # (identity in demo.py:221) is composed as given
    flow_src = ps if fp.points_src_raw is None else _upload(fp.points_src_raw, device)
    # the device-side association enqueues the flow right behind the pair rows, in the same call and ahead of its one
    # read-back (utils_match._match_pcds_device): the frame pair has ONE wait, at its end
    a.flow_request = dict(points=flow_src, labels=ls, pose=pose)
    a.flow_result = None
    a.association_path = None
    pairs, T = yield from utils_match.match_pcds_steps(a, ps, pd, ls, ld, asynchronous)      # utils_track.py:31-35
    if a.association_path == "device" and a.flow_result is not None:
        flow = a.flow_result
    else:
        flow = utils_flow.flow_estimation_torch(a, flow_src, pd, ls, ld, pairs, T, pose)
    out = dict(pairs=pairs, transformations=T, flow=flow, translation_frame=a.translation_frame, association=a.association_path or "host")
    # what the per-segment report (run_sequences), the residual and the objects (run_stream) and the trust bytes (run_sequences) read besides the flow
    if getattr(args, "if_verbose", False) or getattr(args, "residual", None) or getattr(args, "save_trust", None) or getattr(args, "objects", None) or getattr(args, "tracks", None) or getattr(args, "tracks_log", None):
        out.update(labels_src=ls, labels_dst=ld)
    return out


def _native_host(args):
    """One call into the library per frame pair (icpflow_track_frame) unless switched off: `args.native_host = False`, or
    `args.device_association = False` (the host-side association is the Python host's)."""
    return getattr(args, "native_host", True) and getattr(args, "device_association", None) is not False


def register_frame_pair(args, fp, device, gap=None):
    """One frame pair: through `register_frame_pair_native` (one blocking call into the library) where that serves it,
    otherwise `register_frame_pair_steps` driven to its end (every hand-over blocks).  Same result either way."""
    from . import utils_match
    if _native_host(args) and torch.device(device).type == "cuda":
        out = register_frame_pair_native(args, fp, device, gap)
        if _served(out):
            return out
        return _python_host(args, fp, device, gap, out)
    return utils_match.drive(register_frame_pair_steps(args, fp, device, gap))


def register_in_flight_scheduler(args, fps, device, in_flight=4):
    """Register the frame pairs `fps` (an iterable) with up to `in_flight` of them at once: each on its own HIP stream,
    its device -> host hand-overs as asynchronous copies into pinned memory, and ONE host thread that resumes whichever
    frame pair's transfer has landed -- the host half of one frame pair (candidate lists, reject test, assignment) and
    the gaps between its small launches run under the kernels of the others.  Frame pairs are independent
    (main.py:184-215), every one gets exactly the result of `register_frame_pair` (its own random stream included).
    Yields (index, frame pair, result dict) in completion order; the results' tensors are ready on the device."""
    device = torch.device(device)
    # (the streams live as long as the process: pinned staging buffers and workspaces are kept per stream, and pinned
    # memory is expensive to allocate)
    # (per host thread: two threads registering on one device must not share streams)
    pool = _stream_pool.setdefault((device.type, device.index, threading.get_ident()), [])
    while len(pool) < max(int(in_flight), 1):
        pool.append(torch.cuda.Stream(device))
    streams = pool[: max(int(in_flight), 1)]
    free = list(range(len(streams)))
    running = {}                                   # slot -> [index, fp, generator, pending]
    source = enumerate(fps)
    exhausted = False

    def advance(slot):
        idx, fp, gen, _ = running[slot]
        with torch.cuda.stream(streams[slot]):
            try:
                running[slot][3] = next(gen)
                return None
            except StopIteration as done:
                ev = torch.cuda.Event()
                ev.record()
                del running[slot]
                free.append(slot)
                return idx, fp, done.value, ev

    finished = []
    while True:
        while free and not exhausted:
            try:
                idx, fp = next(source)
            except StopIteration:
                exhausted = True
                break
            slot = free.pop()
            running[slot] = [idx, fp, register_frame_pair_steps(args, fp, device, asynchronous=True), None]
            out = advance(slot)
            if out is not None:
                finished.append(out)
        progressed = False
        for slot in list(running):
            if running[slot][3].ready():
                out = advance(slot)
                progressed = True
                if out is not None:
                    finished.append(out)
        for k in range(len(finished) - 1, -1, -1):
            if finished[k][3].query():
                idx, fp, res, _ = finished.pop(k)
                yield idx, fp, res
                progressed = True
        if not running and not finished and exhausted:
            return
        if not progressed:
            # nothing has landed yet: wait for the oldest hand-over instead of spinning on the queries
            if running:
                next(iter(running.values()))[3].get()
            elif finished:
                finished[0][3].synchronize()


_frame_scratch = {}
# what track_frame_native returns when a stage-2 candidate that cannot be in the superset (an over-long cluster) is needed: the
# device-side association of the Python host would give up on this frame pair as well -- go to the host-side association
NEEDS_HOST_ASSOCIATION = "needs the host-side association"


def _served(out):
    return out is not None and out is not NEEDS_HOST_ASSOCIATION


def _python_host(args, fp, device, gap, out):
    """The generators, for a frame pair the native call did not serve (`out`: what it returned)."""
    from . import utils_match
    if out is NEEDS_HOST_ASSOCIATION:
        args = SimpleNamespace(**vars(args))
        args.device_association = False
    return utils_match.drive(register_frame_pair_steps(args, fp, device, gap))


def register_frame_pair_native(args, fp, device, gap=None):
    """One frame pair through icpflow_track_frame: the whole of match_pcds + flow -- the host half included (cluster tables,
    candidate lists, sanity_check, padded batches and their random subsamples, both association stages on the device) -- in ONE
    blocking call into the library, which releases the interpreter lock.  Bit for bit the result of `register_frame_pair` with
    the device-side association (tests/test_gpu_parity.py::test_native_frame_pair_equals_the_python_host).
    -> the result dict, or None when the call cannot serve this frame pair (options outside the single speculative launch, no
    candidate pair at all, more than 512 clusters): the caller takes `register_frame_pair_steps`."""
    a = SimpleNamespace(**vars(args))
    a.translation_frame = frame_translation(args, fp.pose_exact, fp.gap if gap is None else gap)
    device = torch.device(device)
    ps = _input(fp, "points_src", device)
    pd = _input(fp, "points_dst", device)
    pose = torch.from_numpy(fp.pose).to(device)
    flow_src = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
    if fp.labels_src is None and getattr(args, "native_cluster", False):
        # points in: icpflow_track_frame_points clusters the stack itself.  A frame pair it cannot serve goes the way of every
        # other one (the caller's register_frame_pair_steps, which clusters through cluster_frame_pair under the same switch)
        if getattr(args, "cluster", None) not in ("dbscan", "hdbscan"):
            raise ValueError("frame pair without cluster labels: pass precomputed labels_src / labels_dst or set "
                             "args.cluster = 'hdbscan' | 'dbscan'")
        from . import utils_cluster
        par = utils_cluster.cluster_params(SimpleNamespace(epsilon=float(args.epsilon), min_cluster_size=int(args.min_cluster_size),
                                                           num_clusters=int(args.num_clusters), if_hdbscan=args.cluster == "hdbscan"))
        m_src = None if fp.nonground_src is None else torch.as_tensor(fp.nonground_src, device=device).bool()
        m_dst = None if fp.nonground_dst is None else torch.as_tensor(fp.nonground_dst, device=device).bool()
        return track_frame_native(a, ps, pd, None, None, pose, flow_src, cluster=par, mask_src=m_src, mask_dst=m_dst)
    if fp.labels_src is None:
        ls, ld = cluster_frame_pair(args, ps, pd, fp.nonground_src, fp.nonground_dst)
    else:
        ls = _input(fp, "labels_src", device)
        ld = _input(fp, "labels_dst", device)
    return track_frame_native(a, ps, pd, ls, ld, pose, flow_src)


_randperm_ok = None    # None: not checked yet in this process


def randperm_restatement_ok():
    """icpflow_track_frame draws the subsamples of over-long clusters itself: a restatement of torch.randperm's CPU stream
    (MT19937, the 32-bit branch of randperm_cpu; csrc/frame.hip) in place of `torch.randperm` under main.py:139's seed
    (utils_helper.py:198-201).  A torch build that draws differently would give another -- valid, but not reference-identical --
    subsample, silently.  So the first native frame pair of a process compares the two on two (seed, n, take) cases, one of
    them mid-stream; on a mismatch: one warning, and every frame pair of the process goes through the Python host
    (`torch.randperm` itself).  Costs ~0.3 ms once."""
    global _randperm_ok
    if _randperm_ok is None:
        import ctypes
        import warnings
        from . import _lib
        ok = True
        for seed, n, take, skip in ((0, 30552, 2048, 0), (12345, 61849, 10000, 700)):
            g = torch.Generator()
            g.manual_seed(seed)
            if skip:
                torch.randperm(skip, generator=g)
            mt = _lib.Mt19937.from_torch(g)
            want = torch.randperm(n, generator=g)[:take].numpy().astype(np.int32)
            got = np.empty(take, np.int32)
            rc = _lib._L.icpflow_selftest_randperm(ctypes.byref(mt), n, take, got.ctypes.data_as(ctypes.c_void_p))
            ok = ok and rc == 0 and np.array_equal(got, want)
        if not ok:
            warnings.warn("icp_flow_amd: this torch build's randperm does not draw like the library's restatement of it "
                          f"(torch {torch.__version__}); frame pairs are registered through the Python host "
                          "(args.native_host=False), which calls torch.randperm itself", RuntimeWarning, stacklevel=3)
        _randperm_ok = ok
    return _randperm_ok


def track_frame_native(a, ps, pd, ls, ld, pose=None, flow_points=None, seed=0, generator=None, cluster=None, mask_src=None,
                       mask_dst=None):
    """icpflow_track_frame on device tensors: `track(a, ps, pd, ls, ld)` (+ `flow_estimation_torch` of `flow_points` under
    `pose` when given) with `a.translation_frame` set; the random subsamples of over-long clusters are torch.randperm's on a
    generator seeded with `seed` -- or on `generator` (a torch CPU generator, or "global" for torch's own: its state goes in,
    and comes back advanced when the call has served the frame pair).
    cluster (an _lib.ClusterParams; ls / ld None): icpflow_track_frame_points -- the call clusters the stack of both clouds
    itself (mask_src / mask_dst: uint8 or bool device tensors, the non-ground rows, or None) and leaves the labels it used in
    the result under `if_verbose`.
    -> dict(pairs, transformations[, flow]), None (see register_frame_pair_native) or NEEDS_HOST_ASSOCIATION."""
    from . import _lib, utils_match
    import ctypes
    device = ps.device
    max_it, _, stop = utils_match._icp_options(a)
    cur = _lib._current()[-1]
    if not (stop == 0 and 2 <= max_it <= 128 and cur["arith"] == 0 and not (cur["flags"] & _lib.OPT_FLAGS["no_speculative"])):
        return None
    if len(ps) == 0 or len(pd) == 0:
        return None
    if not randperm_restatement_ok():
        return None                     # (the caller's Python host draws with torch.randperm itself)
    _lib.require_gpu(ps, pd, ls, ld, mask_src, mask_dst)
    ps3, pd3 = ps[:, 0:3].contiguous().float(), pd[:, 0:3].contiguous().float()
    if cluster is None:
        ls, ld = ls.contiguous().float(), ld.contiguous().float()
    else:
        ls = torch.empty(len(ps3), dtype=torch.float32, device=device)
        ld = torch.empty(len(pd3), dtype=torch.float32, device=device)
        mask_src = None if mask_src is None else mask_src.to(torch.uint8).contiguous()
        mask_dst = None if mask_dst is None else mask_dst.to(torch.uint8).contiguous()
    rows = torch.empty((1024, 10), dtype=torch.float32, device=device)
    T = torch.empty((1024, 4, 4), dtype=torch.float32, device=device)
    flow = f_pts = f_pose = None
    if flow_points is not None:
        f_pts = ps3 if flow_points is ps else flow_points[:, 0:3].contiguous().float()
        assert len(f_pts) == len(ps3)
        f_pose = pose.to(device).contiguous().float()
        flow = torch.empty((len(ps3), 3), dtype=torch.float32, device=device)
    reg, keep_alive = utils_match._registration(a, device)
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    mt = None
    if generator is not None:
        mt = _lib.Mt19937.from_torch(None if isinstance(generator, str) else generator)
    par = _lib.FrameParams(ctypes.sizeof(_lib.FrameParams), int(seed), ctypes.addressof(mt) if mt is not None else None,
                           int(a.max_points), int(a.min_cluster_size),
                           f32(a.translation_frame), f32(a.thres_box), f32(a.thres_iou), f32(a.thres_rot * 90.0), f32(a.thres_error),
                           1 if getattr(a, "tight_padding", True) else 0, int(getattr(a, "device_association_width", 1024)))
    key = (device.index, _lib.stream_handle(device))
    scratch = _frame_scratch.get(key)
    if scratch is None:
        scratch = _frame_scratch[key] = torch.empty((64 << 20,), dtype=torch.uint8, device=device)
    pairs, need = ctypes.c_int32(0), ctypes.c_size_t(0)
    with _lib.options(teams_half_gpu=not getattr(a, "teams_full_gpu", False), no_shared_scans=not getattr(a, "shared_scans", False),
                      no_stage_overlap=getattr(a, "stage_overlap", None) is False):
        opt = _lib.opt()
        for _ in range(5):   # (the scratch is sized in up to three parts -- fixed, stages, exact stage 2 --, each learnt from a refusal)
            tail = (ctypes.byref(reg), ctypes.byref(par), _lib.ptr(rows), _lib.ptr(T), ctypes.byref(pairs), _lib.ptr(f_pts),
                    _lib.ptr(f_pose), _lib.ptr(flow), _lib.ptr(scratch), scratch.numel(), ctypes.byref(need), _lib.stream(device), opt)
            if cluster is None:
                rc = _lib._L.icpflow_track_frame(_lib.ptr(ps3), _lib.ptr(ls), len(ps3), _lib.ptr(pd3), _lib.ptr(ld), len(pd3), *tail)
            else:
                rc = _lib._L.icpflow_track_frame_points(_lib.ptr(ps3), _lib.ptr(mask_src), len(ps3), _lib.ptr(pd3), _lib.ptr(mask_dst),
                                                        len(pd3), ctypes.byref(cluster), _lib.ptr(ls), _lib.ptr(ld), *tail)
            if rc != -2:
                break
            # (the scratch grows to what this frame pair needs, with some room: the next ones are alike)
            scratch = _frame_scratch[key] = torch.empty((int(need.value * 1.25),), dtype=torch.uint8, device=device)
    if rc != 0:
        msg = _lib._L.icpflow_last_error()
        raise RuntimeError(f"icpflow_track_frame{'_points' if cluster is not None else ''} failed (code {rc}): {msg.decode() if msg else ''}")
    P = int(pairs.value)
    if P == -3:
        return NEEDS_HOST_ASSOCIATION
    if P == -2:
        return None
    if P < 0:
        raise RuntimeError("icpflow_hist_icp abandoned the batch: a wait between workgroups timed out -- a team sharing one "
                           "large pair (GPU shared with another process?); retry, or register with _lib.options(no_teams=True)")
    if mt is not None:
        mt.to_torch(None if isinstance(generator, str) else generator)
    out = dict(pairs=rows[:P], transformations=T[:P], translation_frame=a.translation_frame, association="device")
    if flow is not None:
        out["flow"] = flow
    # what the per-segment report (run_sequences), the residual and the objects (run_stream) and the trust bytes (run_sequences) read besides the flow
    if getattr(a, "if_verbose", False) or getattr(a, "residual", None) or getattr(a, "save_trust", None) or getattr(a, "objects", None) or getattr(a, "tracks", None) or getattr(a, "tracks_log", None):
        out.update(labels_src=ls, labels_dst=ld)
    return out


def register_in_flight(args, fps, device, in_flight=4):
    """Up to `in_flight` frame pairs at once: `register_in_flight_native` (a host thread per frame pair in flight, one blocking
    call into the library each) unless `args.native_host` / `args.device_association` is False -- then the generator-based
    scheduler on one host thread (`register_in_flight_scheduler`).  Yields (index, frame pair, result dict) in completion order."""
    if _native_host(args) and torch.device(device).type == "cuda":
        yield from register_in_flight_native(args, fps, device, in_flight)
    else:
        yield from register_in_flight_scheduler(args, fps, device, in_flight)


class _Worker(threading.Thread):
    """A host thread that lives as long as the process, with its own HIP stream: the library keeps state per host thread (side
    streams, pinned staging) and `track_frame_native` keeps its device scratch per stream -- a thread and a stream per CALL of
    register_in_flight_native would allocate all of that again every time (hipMalloc and hipHostMalloc synchronise the device)."""

    def __init__(self, device):
        super().__init__(daemon=True)
        self.device = device
        self.jobs = queue.Queue()
        self.start()

    def run(self):
        torch.cuda.set_device(self.device)
        stream = torch.cuda.Stream(self.device)
        while True:
            job = self.jobs.get()
            with torch.cuda.stream(stream):
                job(stream)


_workers = {}
_workers_lock = threading.Lock()
_ABANDON_S = 120.0     # a consumer that takes no result for this long has gone (register_in_flight_native)


def register_in_flight_native(args, fps, device, in_flight=4):
    """`register_in_flight` with one HOST THREAD per frame pair in flight, each on its own HIP stream, each frame pair one
    blocking `register_frame_pair_native` call (frame pairs that call cannot serve go through `register_frame_pair_steps` on
    the same thread).  The threads spend their time inside the library with the interpreter lock released; the library chains
    team launches per device whatever thread they come from.  Yields (index, frame pair, result dict) in completion order,
    results complete on the device."""
    from . import utils_match
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    source = enumerate(fps)
    lock = threading.Lock()
    n = max(1, int(in_flight))
    # several frame pairs at once keep the GPU busy by themselves: stage 2's initial poses stay behind stage 1 (the overlap of
    # icpflow_track_frame registers stage 2's whole candidate superset -- extra work that shortens one frame pair on an idle GPU
    # and costs throughput on a busy one: 0.74 -> 0.88 ms per demo frame pair with four in flight when tried); same results
    flight_args = args
    if n > 1 and getattr(args, "stage_overlap", None) is None:
        flight_args = SimpleNamespace(**vars(args))
        flight_args.stage_overlap = False
    out = queue.Queue(maxsize=2 * n + n)     # back-pressure: a slow consumer holds at most ~2 results per worker (+ the end marks)
    stop = threading.Event()                 # the consumer has gone (generator closed, or an error): take no further frame pair

    def deliver(item):
        #  the queue is bounded and the workers outlive the call: a consumer that has gone -- the generator closed, or
        # kept somewhere half-consumed -- must not leave a pooled thread blocked in put() for ever (every later call on this
        # device would queue behind it).  Once `stop` is set the item is dropped; a consumer that takes nothing for
        # _ABANDON_S seconds counts as gone.
        waited = 0.0
        while True:
            try:
                out.put(item, timeout=0.2)
                return
            except queue.Full:
                waited += 0.2
                if stop.is_set() or waited >= _ABANDON_S:
                    stop.set()
                    return

    def job(stream):
        try:
            while True:
                with lock:
                    if stop.is_set():
                        return
                    try:
                        idx, fp = next(source)
                    except StopIteration:
                        return
                res = register_frame_pair_native(flight_args, fp, device)
                if not _served(res):
                    res = _python_host(args, fp, device, None, res)
                stream.synchronize()
                deliver((idx, fp, res))
        except BaseException as e:   # noqa: BLE001  (handed to the consumer)
            deliver(e)
        finally:
            deliver(None)

    with _workers_lock:
        pool = _workers.setdefault(device.index, [])
        while len(pool) < n:
            pool.append(_Worker(device))
        mine = pool[:n]
    for w in mine:
        w.jobs.put(job)
    done, error = 0, None
    try:
        while done < n:
            item = out.get()
            if item is None:
                done += 1
            elif isinstance(item, BaseException):
                error = error or item
                stop.set()
            elif error is None:
                # the result tensors were allocated on the worker's stream: tell the caching allocator that the consumer's
                # stream uses them too, so that a block freed here is not handed out again under a kernel still reading it
                cur = torch.cuda.current_stream(device)
                for v in item[2].values():
                    if isinstance(v, torch.Tensor) and v.is_cuda:
                        v.record_stream(cur)
                yield item
    finally:
        stop.set()                       # (closed early: the workers finish the frame pair they hold and leave)
        waited = 0.0
        while done < n and waited < _ABANDON_S:      # (bounded: a worker stuck inside the library must not hang the consumer too)
            try:
                if out.get(timeout=0.2) is None:
                    done += 1
            except queue.Empty:
                waited += 0.2
    if error is not None:
        raise error


def load_sequence_sample(path, args):
    """The WHOLE sample of a sequence file as the reference's loader returns it (dataset_pca.py:41-69, 103-111): raw_points (in
    the file's own dtype), time_indice, sd_labels, fb_labels, inst_labels, ego_motion_gt, bbox_tsfm, scene_flow (float64) and
    data_path, cropped in x and y like dataset_pca.py:61-64 (args.range_x / range_y; numpy's comparison for the file's dtype).
    A file without `scene_flow` -- every sample of the reference -- gets it from its poses on the GPU
    (utils_loading.scene_flow: icpflow_seq_gt_flow); ours (synthetic.make_sequence) carry the key and keep it.  `nonground`
    is kept when present.  -> dict of numpy arrays."""
    from . import utils_loading
    with np.load(path, allow_pickle=False) as z:
        keys = set(z.files)
        need = ("raw_points", "time_indice", "sd_labels", "fb_labels")
        missing = [k for k in need if k not in keys]
        if missing:
            raise KeyError(f"{path}: not an evaluable sequence sample, missing {missing} (keys: {sorted(keys)})")
        d = {k: np.asarray(z[k]) for k in need}
        for k in ("inst_labels", "ego_motion_gt", "bbox_tsfm", "scene_flow", "nonground"):
            d[k] = np.asarray(z[k]) if k in keys else None
    m = len(d["raw_points"])
    rows = ("raw_points", "time_indice", "sd_labels", "fb_labels", "inst_labels", "scene_flow", "nonground")
    if any(d[k] is not None and len(d[k]) != m for k in rows):                   # dataset_pca.py:54
        raise ValueError(f"{path}: one row per point required in {rows}")
    rx, ry = getattr(args, "range_x", None), getattr(args, "range_y", None)
    if rx is not None and ry is not None:
        raw = d["raw_points"]
        keep = np.logical_and(np.abs(raw[:, 0]) < rx, np.abs(raw[:, 1]) < ry)   # dataset_pca.py:61-64
        for k in rows:
            if d[k] is not None:
                d[k] = d[k][keep]
    if d["scene_flow"] is None:
        if d["inst_labels"] is None or d["bbox_tsfm"] is None or d["ego_motion_gt"] is None:
            raise KeyError(f"{path}: no scene_flow and not all of inst_labels / bbox_tsfm / ego_motion_gt to build it from")
        if d["bbox_tsfm"].shape[1] != d["ego_motion_gt"].shape[0]:              # dataset_pca.py:56
            raise ValueError(f"{path}: bbox_tsfm and ego_motion_gt disagree on the number of frames")
        d["scene_flow"] = utils_loading.scene_flow(d["raw_points"][:, 0:3], d["time_indice"], d["inst_labels"], d["ego_motion_gt"],
                                                   d["bbox_tsfm"])
    else:
        d["scene_flow"] = d["scene_flow"][:, 0:3].astype(np.float64)
    d["data_path"] = path
    return d


ARGO_KEYS = ("pc1", "pc2", "pc1_flows_valid_idx", "pc2_flows_valid_idx", "gt_flow_0_1", "pc1_classes")


def is_argo(path):
    """An Argoverse 2 file as ZeroFlow exports it (dataset_argo.py:36-45) with what its evaluation reads."""
    with np.load(path) as z:
        return all(k in z.files for k in ARGO_KEYS)


def load_argo_sample(path, args, device):
    """One Argoverse 2 file as the reference's other loader returns it (dataset_argo.py:34-101): the file's arrays are uploaded
    once and utils_loading.argo_sample (icpflow_seq_argo_sample) builds the two-frame sample on the device -- frame 0 = pc2's
    valid rows, frame 1 = pc1's with the ground-truth flow, sd = (|flow| > 0.05) and fb from pc1_classes (args.argo_background,
    default utils_loading.ARGO_BACKGROUND_IDXES).  The frame pair is what `load_frame_pair(path)` returns: gap 1, identity
    pose, no non-ground flags -- everything is clustered, as dataset_argo.py:140 does.  There is no CPU path.
    -> (dict of device tensors for calculate_metrics, FramePair)"""
    from . import utils_loading
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ARGO_KEYS if k not in z.files]
        if missing:
            raise KeyError(f"{path}: not an Argoverse 2 sample, missing {missing} (keys: {sorted(z.files)})")
        arrays = {k: np.asarray(z[k]) for k in ARGO_KEYS}
    data = utils_loading.argo_sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"],
                                     arrays["pc1_flows_valid_idx"], arrays["pc2_flows_valid_idx"],
                                     background=getattr(args, "argo_background", None), device=device)
    data["data_path"] = path
    fp = load_frame_pair(path)
    fp.nonground_src = fp.nonground_dst = None
    return data, fp


def _sequence_ground(args, sample, fps):
    """Ground removal stays upstream of the registration: the sample's `nonground` key (load_sequence has put it into the frame
    pairs), else the height threshold of utils_ground.segment_ground_thres on the raw points (utils_ground.py:27-30; under "auto"
    Patchwork++, the other half of the reference's segment_ground, is not applied) when args carries range_z / ground_slack.  Opt-in,
    args.ground == "patchwork": the reference's own segment_ground (Patchwork++ AND the threshold) per frame on the raw points
    of each time_indice, like dataset_pca.py:152-161, whatever key the sample carries.  -> how"""
    from . import utils_ground
    if getattr(args, "ground", "auto") == "patchwork":
        if getattr(args, "range_z", None) is None or getattr(args, "ground_slack", None) is None:
            raise ValueError("ground = 'patchwork' needs range_z and ground_slack (the threshold half of segment_ground)")
        t = sample["time_indice"]
        ng = np.zeros(len(t), dtype=bool)
        for j in np.unique(t):
            ng[t == j] = utils_ground.segment_ground(args, sample["raw_points"][t == j, 0:3])
        for fp in fps:
            fp.nonground_src, fp.nonground_dst = ng[t == fp.gap], ng[t == 0]
        return "patchwork+threshold"
    if sample["nonground"] is not None:
        return "nonground key"
    if getattr(args, "range_z", None) is None or getattr(args, "ground_slack", None) is None:
        return "none"
    ng = utils_ground.segment_ground_thres(args, sample["raw_points"])
    t = sample["time_indice"]
    for fp in fps:
        fp.nonground_src, fp.nonground_dst = ng[t == fp.gap], ng[t == 0]
    return "threshold"


def _sequence_reports(args, path, data, rows, kept):
    """The reference's verbose loop for the frame pairs of one sequence (main.py:262-263: debug_frame per frame, which prints
    its three lines and, under if_verbose, flow_evaluation's): per frame pair the `result` dict of main.py:236-259 from what is
    resident -- the sample's rows of gap j and of frame 0, the labels, pairs and transforms the registration left -- through
    utils_debug.debug_frame.  -> [dict(sequence, gap, frame, lines, segments)]"""
    from . import utils_debug
    out = []
    for fp, reg in sorted(kept, key=lambda x: x[0].gap):
        if "labels_src" not in reg:
            raise RuntimeError("if_verbose: this registration path does not hand the cluster labels over")
        dev = reg["flow"].device
        r = rows[fp.gap]
        result = dict(j=fp.gap, src=data["raw_points"][r], dst=data["raw_points"][rows[0]], pose=torch.from_numpy(fp.pose).to(dev),
                      sd_label=data["sd_labels"][r], fb_label=data["fb_labels"][r], scene_flow=data["scene_flow"][r],
                      src_label=reg["labels_src"], dst_label=reg["labels_dst"], flow=reg["flow"], transformations=reg["transformations"],
                      pairs=reg["pairs"])
        got = utils_debug.debug_frame(args, result)
        out.append(dict(sequence=path, gap=fp.gap, **got))
    return out


def worst_segments(reports, threshold=2.0):
    """The segments of run_sequences' reports whose EPE exceeds `threshold`, worst first: [dict(sequence, gap, label, n, epe,
    matched_label, translation, rotation_zyx_deg)] (what --report writes)."""
    rows = [dict(sequence=r["sequence"], gap=r["gap"], **seg) for r in reports for seg in r["segments"].worst(threshold)]
    return sorted(rows, key=lambda x: -x["epe"])


def _pca_inputs(args, path, device, F, ground, pose_sources):
    """run_sequences, a Waymo / nuScenes file: what is resident before the clock starts.  -> (data, frame pairs, rows per frame)"""
    sample = load_sequence_sample(path, args)
    fps = load_sequence(path, args)
    t = sample["time_indice"]
    counts = [int((t == j).sum()) for j in range(F)]
    if len(fps) != F - 1 or [len(fp.points_src) for fp in fps] != counts[1:] or (fps and len(fps[0].points_dst) != counts[0]):
        raise ValueError(f"{path}: the frame pairs do not cover the sample's points (num_frames {F}, points per frame {counts})")
    how = _sequence_ground(args, sample, fps)
    ground[how] = ground.get(how, 0) + 1
    for fp in fps:
        pose_sources[fp.pose_source] = pose_sources.get(fp.pose_source, 0) + 1
    # resident before the clock starts: what the evaluation reads besides the flows, and where each frame's rows are
    on = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device).to(dt)   # noqa: E731
    data = dict(raw_points=on(sample["raw_points"][:, 0:3], torch.float64 if sample["raw_points"].dtype == np.float64 else torch.float32),
                time_indice=on(utils_eval.narrow_time_indices(t, F), torch.int32), sd_labels=on(sample["sd_labels"], torch.int32),
                fb_labels=on(sample["fb_labels"], torch.int32), scene_flow=on(sample["scene_flow"], torch.float64))
    if not (np.isin(sample["sd_labels"], (0, 1)).all() and np.isin(sample["fb_labels"], (0, 1)).all()):
        data["sd_labels"], data["fb_labels"] = utils_eval._binary_labels(sample["sd_labels"], device), utils_eval._binary_labels(sample["fb_labels"], device)
    rows = [on(np.flatnonzero(t == j), torch.int64) for j in range(F)]
    return data, fps, rows


def _argo_inputs(args, path, device, ground, pose_sources):
    """run_sequences, an Argoverse 2 file: the sample (built on the device), its one frame pair, and the rows of its two
    frames -- two contiguous ranges.  -> (data, frame pairs, rows per frame)"""
    data, fp = load_argo_sample(path, args, device)
    m2, m = len(fp.points_dst), len(data["time_indice"])
    if m != m2 + len(fp.points_src):
        raise ValueError(f"{path}: the frame pair does not cover the sample's points")
    ground["none"] = ground.get("none", 0) + 1
    pose_sources[fp.pose_source] = pose_sources.get(fp.pose_source, 0) + 1
    rows = [torch.arange(0, m2, device=device), torch.arange(m2, m, device=device)]
    return data, [fp], rows


SPLITS = ("train", "val", "test")


def flow_file(path, estimated_poses=False):
    """Where a sequence's flow is saved, --if_save of the reference (main.py:265-280) by `_pose_file`'s idea instead of its
    substring replacement: the LAST directory component that is a split (train / val / test) or starts with one plus "_"
    (the Argoverse tree's val_zero_flow) gets "_icp_flow" (estimated ego poses) or "_icp_flow_ego" (ground-truth poses)
    after the split's name: .../val/x.npz -> .../val_icp_flow_ego/x.npz, .../val_zero_flow/log/x.npz ->
    .../val_icp_flow_ego_zero_flow/log/x.npz.  No such component: ValueError."""
    parts = os.path.normpath(path).split(os.sep)
    tag = "_icp_flow" if estimated_poses else "_icp_flow_ego"
    for k in range(len(parts) - 2, -1, -1):
        for split in SPLITS:
            if parts[k] == split or parts[k].startswith(split + "_"):
                return os.sep.join(parts[:k] + [split + tag + parts[k][len(split):]] + parts[k + 1:])
    raise ValueError(f"{path}: no split directory (train / val / test, or one of them plus '_...') to put the saved flow next to")


def save_sequence_flow(path, flow_seq, fps, F, trust=None, trust_params=None):
    """np.savez_compressed to flow_file(path), the reference's keys (main.py:281-284): scene_flow float64 [m,3] (the float32
    flows widened; zeros for frame 0; the rows of the sample as loaded), ego_motion float64 [F,4,4] (the poses the frame pairs
    were registered with; identity for frame 0).  trust (uint8 [m], one byte per row of scene_flow: utils_eval.flow_trust's;
    zeros for frame 0) adds two keys that the reference does not write: `trust`, and `trust_params`, a JSON string of
    trust_params (a dict: what the bytes were made with).  -> the file written"""
    poses = np.stack([np.eye(4)] * F)
    for fp in fps:
        poses[fp.gap] = fp.pose_exact
    estimated = any(fp.pose_source in ("pose_file", "ego_motion", "estimate") for fp in fps)
    out = flow_file(path, estimated)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    arrays = dict(scene_flow=flow_seq.to(torch.float64).cpu().numpy(), ego_motion=poses)
    if trust is not None:
        if trust.dtype != torch.uint8 or tuple(trust.shape) != (flow_seq.shape[0],):
            raise ValueError(f"save_sequence_flow: trust {tuple(trust.shape)} {trust.dtype} for {flow_seq.shape[0]} rows of uint8")
        arrays.update(trust=trust.cpu().numpy(), trust_params=np.array(json.dumps(dict(trust_params or {}), sort_keys=True)))
    np.savez_compressed(out, **arrays)
    return out


TRUST_RADIUS = 2.0  # metres: the residual's radius behind run_sequences' trust bytes (--residual's own default)
RECORD_HEAD = 6     # file index, kept0, frame pairs, wall time, evaluation time, save time (the three in microseconds)


def sequence_record(index, F, table, kept0, n_pairs, us, classes=None, *, buckets=None):
    """One file's numbers as int64 words: RECORD_HEAD words, the F * 36 words of sequence_table (the sums of e as their bits),
    then the class table's words when there is one, then the bucket table's (`buckets`, a utils_eval.BucketTable) when there
    is one.  `us`: (wall, evaluation, save) in microseconds."""
    head = np.array([index, kept0, n_pairs] + [int(round(u)) for u in us], dtype=np.int64)
    parts = [head, np.ascontiguousarray(table, dtype=np.int64).reshape(F * 36)]
    if classes is not None:
        parts.append(classes.words())
    if buckets is not None:
        parts.append(buckets.words())
    return np.concatenate(parts)


def merge_sequence_records(args, records, total, rank=0, world=1, group=None, device=None, class_shape=None, *, bucket_shape=None):
    """The end of a sharded run_sequences, with no GPU work of its own: ONE all_gather of every rank's records (padded to
    the largest share with rows whose file index is -1; on the device under NCCL, on the host under gloo, chosen as
    run_stream chooses), then -- on every rank -- update_meters and ClassTable.add replayed IN FILE ORDER, which is what a
    single process does: meters and class table are bit-identical to its, whatever the world size and however uneven the
    shares.  records: this rank's sequence_record()s; total: files in all; class_shape: (G, S, E) when the records carry a
    class table.  -> (metrics, ClassTable or None, rows [total, RECORD_HEAD] of the records' heads in file order).
    bucket_shape: (G, S) when the records carry a bucket table behind that; BucketTable.add is replayed in file order like the
    rest, and the result has a fourth entry, the BucketTable."""
    F = int(args.num_frames)
    class_words = class_shape[0] * class_shape[1] * (class_shape[2] + 2) if class_shape else 0
    words = RECORD_HEAD + F * 36 + class_words + (bucket_shape[0] * bucket_shape[1] * 3 if bucket_shape else 0)
    share = -(-total // world) if total else 0
    local = np.full((share, words), -1, dtype=np.int64)
    if len(records) > share or any(len(r) != words for r in records):
        raise ValueError(f"rank {rank}: {len(records)} records for a share of {share}, or a record that is not {words} words")
    for k, r in enumerate(records):
        local[k] = r
    if world > 1:
        import torch.distributed as dist
        on_gpu = dist.get_backend(group) == "nccl"
        mine = torch.from_numpy(local).to(device if on_gpu else "cpu")
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine, group=group)
        every = torch.cat(parts).cpu().numpy()
    else:
        every = local
    every = every[every[:, 0] >= 0]
    every = every[np.argsort(every[:, 0], kind="stable")]
    if not np.array_equal(every[:, 0], np.arange(total)):
        raise RuntimeError(f"the gathered records do not cover files 0 .. {total - 1} once each: {every[:, 0].tolist()}")
    metrics = utils_eval.new_metric_table(F)
    classes = utils_eval.ClassTable.zeros(*class_shape) if class_shape else None
    buckets = utils_eval.BucketTable.zeros(*bucket_shape) if bucket_shape else None
    for row in every:
        table = np.ascontiguousarray(row[RECORD_HEAD:RECORD_HEAD + F * 36]).reshape(F, 6, 6)
        esum = np.ascontiguousarray(table[:, :, 1]).view(np.float64)
        utils_eval.update_meters(args, metrics, table, esum, int(row[1]))
        if classes is not None:
            classes.add(utils_eval.ClassTable.from_words(row[RECORD_HEAD + F * 36:RECORD_HEAD + F * 36 + class_words], *class_shape, kept0=int(row[1])))
        if buckets is not None:
            buckets.add(utils_eval.BucketTable.from_words(row[RECORD_HEAD + F * 36 + class_words:], *bucket_shape, kept0=int(row[1])))
    if bucket_shape:
        return metrics, classes, every[:, :RECORD_HEAD], buckets
    return metrics, classes, every[:, :RECORD_HEAD]


def run_sequences(args, paths, device, in_flight=1, dataset="pca", rank=0, world=1, group=None):
    """Evaluate sequence files by the reference's protocol (main.py:173-296).  Per file: the sample
    (`load_sequence_sample`) and its num_frames - 1 frame pairs (`load_sequence`), registered by the existing path
    (`register_frame_pair`, or `register_in_flight` with in_flight > 1); the flows are put into the sequence's flow ON THE
    DEVICE (zeros for frame 0, main.py:217-260) and `utils_eval.calculate_metrics` takes it from there: one launch pair, one
    read-back of the table.  args: the registration's (default_args) plus num_frames, range_x, range_y, range_z,
    ground_slack, eval_ground.
    -> dict(metrics = the reference's meters, sequences, frame_pairs, ms_per_sequence (registration + evaluation, the
    sample's evaluation inputs resident beforehand like the loader's work), ms_eval_per_sequence, ground, pose_sources).
    With args.if_verbose (absent = False): after a sequence's evaluation the reference's per-frame lines and per-segment
    report of each of its frame pairs (utils_debug.debug_frame, utils_flow.flow_evaluation; printed as the reference prints
    them), returned under `segments` and timed on their own as ms_report_per_sequence; the other two times keep their meaning.
    dataset="argo" (main.py:156-159, `--dataset argo`): every file is one Argoverse 2 sample of two frames (`load_argo_sample`:
    the sample and its labels built on the device), its one frame pair registered as above; no ground removal, whatever
    args.ground says (dataset_argo.py:140).
    args.class_table (absent = off; dataset="argo" only): utils_eval.class_table per file, one more pass and one more small
    read-back inside ms_eval_per_sequence, accumulated in file order -> `class_table` (a utils_eval.ClassTable) and `threeway`.
    args.bucket_table (absent = off; dataset="argo" only): utils_eval.bucket_table per file, one more pass and one more small
    read-back inside ms_eval_per_sequence, accumulated in file order -> `bucket_table` (a utils_eval.BucketTable) and
    `bucketed_epe` (utils_eval.bucketed_epe of it); independent of args.class_table.
    args.save_flows (absent = False): after a sequence's evaluation its flow and poses are written to `flow_file(path)`
    (`save_sequence_flow`) -- outside the two times above, reported as ms_save_per_sequence.
    rank / world / group: the files are dealt round-robin (`shard_round_robin`), every rank keeps one record per file and
    `merge_sequence_records` gathers them once at the end and replays them in file order: `metrics`, `class_table`, the
    counts and the times are those of the whole run on every rank, bit for bit the single process's; ground and pose_sources
    are this rank's, every rank saves its own files, and if_verbose is refused (merging the reports is not built).
    args.save_trust = True or (x, y, z) (absent = off; needs args.save_flows): one trust byte per point beside the saved flow --
    `frame_trust` per frame pair at TRUST_RADIUS metres (True: the residual alone; an origin: the line of sight from there as
    well), the bytes put into a uint8 [m] by the rows of their frame (zeros for frame 0) and written as the file's `trust` and
    `trust_params` keys.  After the evaluation and outside its times: -> `trust` (the counts over this rank's files, kept_share,
    params) and `ms_trust_per_sequence`; without the attribute the result and the files are what they were."""
    device = torch.device(device)
    F = int(args.num_frames)
    if dataset not in ("pca", "argo"):
        raise ValueError(f"dataset must be 'pca' or 'argo' (got {dataset!r})")
    if dataset == "argo" and F != 2:
        raise ValueError(f"an Argoverse 2 sample has two frames (num_frames {F})")
    with_classes = bool(getattr(args, "class_table", None))
    if with_classes and dataset != "argo":
        raise ValueError("class_table goes with dataset='argo' (the other files' sem_labels have no names in the reference)")
    with_buckets = bool(getattr(args, "bucket_table", None))
    if with_buckets and dataset != "argo":
        raise ValueError("bucket_table goes with dataset='argo' (the classes and the buckets are Argoverse 2's)")
    saving = bool(getattr(args, "save_flows", False))
    verbose = bool(getattr(args, "if_verbose", False))
    if world > 1 and verbose:
        raise ValueError("if_verbose under more than one rank: merging the reports is not built")
    trusting = getattr(args, "save_trust", None)
    trusting = None if trusting is None or trusting is False else trusting
    if trusting is not None and not saving:
        raise ValueError("args.save_trust needs args.save_flows: the bytes go into the saved flow's file")
    trust_origin = None if trusting is None or trusting is True else tuple(float(v) for v in trusting)
    if trust_origin is not None and len(trust_origin) != 3:
        raise ValueError(f"args.save_trust: True or an origin (x, y, z), got {trusting!r}")
    trust_counts, trust_times, trust_params = utils_eval.TrustCounts(), [], None
    if trusting is not None:
        from . import _lib
        trust_params = dict(radius=TRUST_RADIUS, origin=None if trust_origin is None else list(trust_origin), **_lib.TrustParams.defaults().as_dict())
        if trust_origin is not None:
            trust_params["sight"] = _lib.SightParams.defaults().as_dict()
    paths = list(paths)
    mine = shard_round_robin(list(enumerate(paths)), rank, world)        # (file index, path)
    class_shape = (utils_eval.ARGO_CLASS_ROWS, len(utils_eval.ARGO_SPEED_EDGES) + 1, len(utils_eval.ARGO_ERROR_EDGES) + 1) if with_classes else None
    metrics = utils_eval.new_metric_table(F)
    classes = utils_eval.ClassTable.zeros(*class_shape) if with_classes else None
    bucket_shape = (utils_eval.ARGO_CLASS_ROWS, len(utils_eval.ARGO_BUCKET_EDGES) + 1) if with_buckets else None
    buckets = utils_eval.BucketTable.zeros(*bucket_shape) if with_buckets else None
    times, eval_times, save_times, n_pairs, ground, pose_sources = [], [], [], 0, {}, {}
    segments, report_times, records = [], [], []
    for index, path in mine:
        if dataset == "argo":
            data, fps, rows = _argo_inputs(args, path, device, ground, pose_sources)
        else:
            data, fps, rows = _pca_inputs(args, path, device, F, ground, pose_sources)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        flow_seq = torch.zeros((len(data["time_indice"]), 3), dtype=torch.float32, device=device)
        if int(in_flight) > 1:
            done = register_in_flight(args, fps, device, in_flight)
        else:
            done = ((k, fp, register_frame_pair(args, fp, device)) for k, fp in enumerate(fps))
        kept, pairs_here = [], 0
        for _, fp, out in done:
            flow_seq.index_copy_(0, rows[fp.gap], out["flow"].to(torch.float32))
            pairs_here += 1
            if verbose or trusting is not None:
                kept.append((fp, out))
        n_pairs += pairs_here
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        if world == 1:
            utils_eval.calculate_metrics(args, data, flow_seq, metrics)     # (its read-back of the table is the synchronisation)
        else:                                                               # the same table, kept for the replay in file order
            table, esum, kept0 = utils_eval.checked_sequence_table(args, data, flow_seq)
        one = utils_eval.class_table(args, data, flow_seq) if with_classes else None
        if world == 1 and with_classes:
            classes.add(one)
        one_b = utils_eval.bucket_table(args, data, flow_seq) if with_buckets else None
        if world == 1 and with_buckets:
            buckets.add(one_b)
        t2 = time.perf_counter()
        times.append((t2 - t0) * 1e3)
        eval_times.append((t2 - t1) * 1e3)
        if verbose:
            segments.extend(_sequence_reports(args, path, data, rows, kept))
            report_times.append((time.perf_counter() - t2) * 1e3)
        trust_seq = None
        if trusting is not None:                  # (outside the two times above: the registrations' results are resident)
            torch.cuda.synchronize(device)
            t4 = time.perf_counter()
            trust_seq = torch.zeros(flow_seq.shape[0], dtype=torch.uint8, device=device)      # frame 0: zeros
            for fp, out in kept:
                bytes_, counted = frame_trust(fp, out, device, TRUST_RADIUS, trust_origin)
                trust_seq.index_copy_(0, rows[fp.gap], bytes_)
                trust_counts.add(counted)
            torch.cuda.synchronize(device)
            trust_times.append((time.perf_counter() - t4) * 1e3)
        if saving:
            t3 = time.perf_counter()
            save_sequence_flow(path, flow_seq, fps, F, trust=trust_seq, trust_params=trust_params)
            save_times.append((time.perf_counter() - t3) * 1e3)
        if world > 1:
            records.append(sequence_record(index, F, table, kept0, pairs_here,
                                           (times[-1] * 1e3, eval_times[-1] * 1e3, save_times[-1] * 1e3 if saving else 0.0), one, buckets=one_b))
    if world > 1:
        merged = merge_sequence_records(args, records, len(paths), rank, world, group, device, class_shape, bucket_shape=bucket_shape)
        metrics, classes, heads = merged[:3]
        buckets = merged[3] if with_buckets else None
        n_pairs = int(heads[:, 2].sum())
        times, eval_times = (heads[:, 3] * 1e-3).tolist(), (heads[:, 4] * 1e-3).tolist()
        save_times = (heads[:, 5] * 1e-3).tolist() if saving else []
    res = dict(metrics=metrics, sequences=len(times), frame_pairs=n_pairs, ms_per_sequence=sum(times) / max(len(times), 1),
               ms_eval_per_sequence=sum(eval_times) / max(len(eval_times), 1),
               ground="+".join(sorted(ground)) if ground else "none", pose_sources=pose_sources)
    if verbose:
        res.update(segments=segments, ms_report_per_sequence=sum(report_times) / max(len(report_times), 1))
    if saving:
        res.update(ms_save_per_sequence=sum(save_times) / max(len(save_times), 1))
    if trusting is not None:                      # (this rank's files, like ground and pose_sources)
        res.update(trust=dict(trust_counts.summary(), params=trust_params), ms_trust_per_sequence=sum(trust_times) / max(len(trust_times), 1))
    if with_classes:
        res.update(class_table=classes, threeway=classes.threeway(utils_eval.ARGO_META_GROUPS["BACKGROUND"]))
    if with_buckets:
        res.update(bucket_table=buckets, bucketed_epe=utils_eval.bucketed_epe(buckets))
    return res


def _by_sample(items, args, sample_of, samples):
    """run_stream's frame pairs, in their order, with the samples they are gaps of written down as they go by: sample_of[number
    of the frame pair] = its sample, samples[sample] = dict(sample, size, outs).  The frame pairs of one sequence file are one
    sample (load_sequence tags them with the file's path), and so are consecutive FramePair objects that carry the same tag; a
    frame-pair file or an untagged FramePair is a sample of its own.  Frame pairs of one sample that disagree on the rows of the
    shared sweep are a ValueError before any of them is registered."""
    number, k, begun = 0, 0, 0
    while k < len(items):
        item = items[k]
        if isinstance(item, FramePair):
            j = k + 1
            while item.sequence is not None and j < len(items) and isinstance(items[j], FramePair) and items[j].sequence == item.sequence:
                j += 1
            groups, k = [list(items[k:j])], j
        else:
            fps, k = load_any(item, args), k + 1
            tagged = bool(fps) and fps[0].sequence is not None and all(fp.sequence == fps[0].sequence for fp in fps)
            groups = [fps] if tagged else [[fp] for fp in fps]
        for fps in groups:
            if not fps:
                continue
            rows = sorted({len(fp.points_dst) for fp in fps})
            if len(rows) > 1:
                raise ValueError(f"object tracks: the frame pairs of {fps[0].sequence!r} disagree on the rows of the shared sweep ({rows}): "
                                 "they are not the gaps of one sample")
            s, begun = begun, begun + 1                       # (samples are numbered in the order they begin)
            samples[s] = dict(sample=s, size=len(fps), outs={})
            for fp in fps:
                sample_of[number] = s
                number += 1
                yield fp


def run_stream(args, paths, device, rank=0, world=1, repeat=1, group=None, register_fn=None, in_flight=1):
    """Register this rank's share of `paths`; -> summary dict (identical on every rank).
    ms / frame pair is the mean wall time per pair, host -> device upload of the clouds included
    (the stream hands over host buffers); frame_pairs_per_s uses the slowest rank's total.
    `register_fn(args, fp, device) -> dict(pairs, transformations, flow)` defaults to the HIP path
    (`register_frame_pair`); the CPU tests of the sharding logic pass the oracle here.
    in_flight > 1 (HIP path only): that many frame pairs at once (`register_in_flight`: one stream and one host thread each, a
    blocking call into the library per frame pair; or the one-thread scheduler with asynchronous hand-overs); ms / frame pair is then the wall time of the whole share over its frame pairs --
    throughput of the stream, not the latency of one pair.
    Every registered frame pair -- in flight: once delivered -- then goes to the judges that `args` switches on, outside the
    timed region of one pair at a time (in flight, ms / frame pair is the wall time of the share and includes their work).
    There are seven, each described at its class in pair_judges.py: args.residual (ResidualJudge), args.residual_segments
    (SegmentJudge), args.residual_sight (SightJudge), args.residual_trust (TrustJudge), args.objects (ObjectJudge), args.tracks
    (TrackJudge) and args.tracks_log (LogTrackJudge, which also closes its log once the last frame pair is accounted).  A judge is handed the frame pair's number in this rank's share (in flight: `register_in_flight`'s index) and
    keeps what it finds under it, so no result depends on the order in which frame pairs complete; after the one all_reduce
    each adds its keys to the summary, in the order above, and writes its file."""
    import torch.distributed as dist
    device = torch.device(device)
    pipelined = int(in_flight) > 1 and register_fn is None
    register_fn = register_fn or register_frame_pair

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    mine = shard_round_robin(paths, rank, world)
    meter = utils_eval.AverageMeter()
    times, matched, accounted = [], 0, 0
    pose_sources, scores = {}, {}        # scores: frame pair -> its five metrics and its rows
    every = (fp for path in mine for fp in ([path] if isinstance(path, FramePair) else load_any(path, args)))   # a sequence file yields one pair per gap
    # the judges: every constructor checks its attributes of `args`, so the order here decides which error wins
    residual = ResidualJudge(args, world, device)
    segments = SegmentJudge(args, world, device, residual)
    sight = SightJudge(args, world, device, segments)
    trust = TrustJudge(args, world, device, segments, sight)
    objects = ObjectJudge(args, world, device)
    sample_of, samples = {}, {}      # frame pair -> its sample; sample -> its frame pairs: _by_sample fills them, the tracks empty them
    tracks = TrackJudge(args, world, device, objects, sample_of, samples)
    if tracks.on:
        every = _by_sample(mine, args, sample_of, samples)
    log = LogTrackJudge(args, world, device, objects)
    judges = [j for j in (residual, segments, sight, trust, objects, tracks, log) if j.on]

    def account(fp, out, index=None):
        nonlocal matched, accounted
        number, accounted = (accounted if index is None else index), accounted + 1
        for j in judges:
            j.account(number, fp, out)
        pose_sources[fp.pose_source] = pose_sources.get(fp.pose_source, 0) + 1
        matched += int(out["pairs"].shape[0])
        if fp.gt_flow is not None:
            m = utils_eval.compute_epe_test(out["flow"].cpu().numpy(), fp.gt_flow, fp.mask)
            n = int((np.asarray(fp.mask) > 0).sum()) if fp.mask is not None else len(fp.gt_flow)
            scores[number] = (*m, n)

    if pipelined:
        sync()
        t0 = time.perf_counter()
        n = 0
        for index, fp, out in register_in_flight(args, every, device, in_flight):
            account(fp, out, index)
            n += 1
        sync()
        times = [(time.perf_counter() - t0) * 1e3 / max(n, 1)] * n
    else:
        for fp in every:
            if repeat > 1:
                register_fn(args, fp, device)                   # untimed pass: page-in, allocator
            sync()
            t0 = time.perf_counter()
            for _ in range(repeat):
                out = register_fn(args, fp, device)
            sync()
            times.append((time.perf_counter() - t0) / repeat * 1e3)
            account(fp, out)
    if log.on:
        log.close()
    for number in sorted(scores):       # (the meter's sums in the order of the frame pairs, whatever order they completed in)
        meter.update(*scores[number])
    # five weighted sums + point count + time + frame pairs + matches (+ what a judge adds): one small all_reduce
    local = [getattr(meter, m + "_sum") for m in utils_eval.METRIC_NAMES] + [meter.num, sum(times), len(times), matched]
    riding = [(j, j.reduce_words()) for j in judges if hasattr(j, "reduce_words")]
    local += [w for _, words in riding for w in words]
    on_gpu = world > 1 and dist.get_backend(group) == "nccl"
    tot = torch.tensor(local, dtype=torch.float64, device=device if on_gpu else "cpu")
    tmax = torch.tensor([sum(times)], dtype=torch.float64, device=tot.device)
    if world > 1:
        dist.all_reduce(tot, group=group)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX, group=group)
    tot = tot.tolist()
    n_pts, n_fp, at = tot[5], int(tot[7]), 9
    for j, words in riding:
        j.take_words(tot[at: at + len(words)])
        at += len(words)
    out = {"frame_pairs": n_fp, "matched_cluster_pairs": int(tot[8]), "n_gpus": world,
           "ms_per_frame_pair": tot[6] / max(n_fp, 1),
           "frame_pairs_per_s": n_fp / (float(tmax.item()) * 1e-3) if n_fp else 0.0,
           "evaluated_points": int(n_pts),
           "pose_sources": pose_sources}     # (this rank's frame pairs: "ego_motion_gt" = ground-truth ego poses were used)
    if n_pts > 0:
        out.update({m: tot[k] / n_pts for k, m in enumerate(utils_eval.METRIC_NAMES)})
    for j in judges:
        j.summarise(out)
    return out


def argument_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("directory")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--in-flight", type=int, default=1, help="frame pairs registered at once (a stream and a host thread each)")
    def flag(text):      # (type=bool would read every non-empty string, "False" included, as True)
        if text.lower() in ("1", "true", "yes", "on"):
            return True
        if text.lower() in ("0", "false", "no", "off"):
            return False
        raise argparse.ArgumentTypeError(f"expected true/false, got {text!r}")
    for k, v in DEFAULT_ARGS.items():
        kind = str if k == "cluster" else flag if isinstance(v, bool) else float if isinstance(v, float) or v is None else type(v)
        ap.add_argument("--" + k.replace("_", "-"), type=kind, default=v)
    ap.add_argument("--pose-source", choices=POSE_SOURCES, default=None,
                    help="ego poses of sequence files (default auto; estimate = scan-to-map odometry on the GPU)")
    ap.add_argument("--save-poses", action="store_true", help="with --pose-source estimate: write the <split>_pose files")
    ap.add_argument("--ego-deskew", action="store_true",
                    help="with --pose-source estimate: deskew every frame by the file's point_time key (stamps in [0, 1] over a sweep)")
    ap.add_argument("--ego-fixed-threshold", type=float, default=0.0, metavar="X",
                    help="with --pose-source estimate: sigma = X metres on every frame instead of the adaptive threshold (0 = adaptive)")
    ap.add_argument("--protocol", choices=("reference",), default=None,
                    help="reference: evaluate sequence files by the reference's table of 6 classes x (num_frames + 1) rows")
    ap.add_argument("--dataset", choices=("pca", "argo"), default="pca",
                    help="--protocol reference: pca = Waymo / nuScenes sequence files; argo = Argoverse 2 files as ZeroFlow exports "
                         "them, one two-frame sample each (main.py:156-159)")
    ap.add_argument("--num-frames", type=int, default=None,
                    help="--protocol reference: frames per sequence (main.py:67; default 5, with --dataset argo 2 and nothing else)")
    ap.add_argument("--range-z", type=float, default=0.0, help="--protocol reference: ground <= range_z (main.py:73)")
    ap.add_argument("--ground-slack", type=float, default=0.3, help="--protocol reference (main.py:113)")
    ap.add_argument("--eval-ground", action="store_true", help="--protocol reference: evaluate ground points too (main.py:115)")
    ap.add_argument("--ground", choices=("auto", "patchwork"), default="auto",
                    help="--protocol reference: auto = the file's nonground key, else the height threshold; patchwork = "
                         "Patchwork++ AND the threshold per frame on the GPU (utils_ground.py:16-23)")
    ap.add_argument("--if-verbose", action="store_true",
                    help="--protocol reference: print the per-frame and per-segment lines of the reference's --if_verbose (main.py:117)")
    ap.add_argument("--native-cluster", action="store_true",
                    help="with --cluster: frame pairs without labels are clustered inside the library (icpflow_cluster_pcd / "
                         "icpflow_track_frame_points) instead of by the Python clustering; off by default")
    ap.add_argument("--report", metavar="FILE", default=None,
                    help="--protocol reference: write a JSON list of the segments with EPE above --report-epe, worst first")
    ap.add_argument("--report-epe", type=float, default=2.0, help="threshold of --report in metres (utils_flow.py:112)")
    ap.add_argument("--class-table", choices=("meta", "fine"), default=None,
                    help="--protocol reference --dataset argo: per meta category (fine: and per category) and speed bucket n, EPE, "
                         "speed and the error splits, and the three-way EPE, after the reference's table")
    ap.add_argument("--bucketed-epe", action="store_true",
                    help="--protocol reference --dataset argo: the bucket-normalised EPE per class of the Argoverse 2 2024 challenge "
                         "(static EPE and speed-normalised dynamic EPE over 51 speed buckets), after the reference's table; the "
                         "challenge's region is --range-x 35 --range-y 35")
    ap.add_argument("--save-flows", action="store_true",
                    help="--protocol reference: write every sequence's flow and poses next to its split (<split>_icp_flow[_ego], main.py:265-284)")
    ap.add_argument("--residual", type=float, nargs="?", const=2.0, default=None, metavar="R",
                    help="judge the flow without ground truth: the nearest-neighbour residual of the warped source against the "
                         "destination, truncated at R metres (2.0 when given bare), before and after the registration, both "
                         "directions (Chamfer); not with --protocol reference")
    ap.add_argument("--residual-segments", nargs="?", const=True, default=None, metavar="FILE",
                    help="with --residual: the residual per segment (cluster) of every frame pair's source, before and after the "
                         "flow; lists the segments whose mean distance under the flow exceeds 0.1 m, worst first (FILE: the "
                         "whole list as JSON); one process only")
    ap.add_argument("--residual-sight", type=float, nargs="*", default=None, metavar="X",
                    help="with --residual-segments: the line-of-sight check of every listed segment against a depth image of the "
                         "destination sweep -- 'seen through' (the flow put it where the sweep saw free space), 'lost from view' "
                         "(occluded, no return, out of range) or 'undecided'; X Y Z: the sensor's position in the frame of the "
                         "points (bare: 0 0 0)")
    ap.add_argument("--residual-trust", action="store_true",
                    help="with --residual-segments: one trust byte per source point (near / far and how the sweep saw it, its "
                         "segment's verdict, KEEP), counted over the run; uses the line of sight iff --residual-sight is given; "
                         "with gt_flow in the files, the EPE of the kept and of the dropped rows")
    ap.add_argument("--save-trust", type=float, nargs="*", default=None, metavar="X",
                    help="with --save-flows: write one trust byte per point into the saved flow's file (keys trust, trust_params), "
                         "from the residual at 2 m; X Y Z: the sensor's position in the frame of the points, to use the line of "
                         "sight as well (bare: the residual alone)")
    ap.add_argument("--objects", nargs="?", const=True, default=None, metavar="FILE",
                    help="object pseudo labels: per matched cluster pair an oriented box, a velocity, a heading and the distance "
                         "of the moved box's centre from the matched destination cluster's (FILE: one JSON line per frame pair); "
                         "one process only; not with --protocol reference")
    ap.add_argument("--sweep-seconds", type=float, default=utils_objects.SWEEP_SECONDS, metavar="S",
                    help="with --objects: the time between two sweeps; a frame pair `gap` sweeps apart spans gap * S seconds")
    ap.add_argument("--objects-min-speed", type=float, default=utils_objects.MIN_SPEED, metavar="V",
                    help="with --objects: an object moves when its xy speed reaches V m/s")
    ap.add_argument("--tracks", nargs="?", const=True, default=None, metavar="FILE",
                    help="object tracks: the objects of a multi-frame sample linked across its gaps (they share the sweep of frame 0), "
                         "per track a velocity fitted over all gaps, the residuals from it, a size over all views and whether the "
                         "gaps agree on one constant velocity (FILE: one JSON line per sample); uses --sweep-seconds and "
                         "--objects-min-speed; one process only; not with --protocol reference")
    ap.add_argument("--tracks-min-iou", type=float, default=utils_tracks.MIN_IOU, metavar="I",
                    help="with --tracks: a cluster inherits a track when the two are each other's largest overlap at IoU >= I")
    ap.add_argument("--tracks-max-residual", type=float, default=utils_tracks.MAX_RESIDUAL, metavar="M",
                    help="with --tracks: a track is consistent when no gap's displacement lies more than M metres off the fitted velocity")
    ap.add_argument("--tracks-repair", action="store_true",
                    help="with --tracks: a gap that alone breaks its track's constant velocity is registered again from the motion the other "
                         "gaps predict, and the new pose replaces the old one where the data prefer it (transforms, pair rows, flow, objects "
                         "and tracks of that gap); not with --tracks-log, not with --protocol reference")
    ap.add_argument("--tracks-fill", action="store_true",
                    help="with --tracks: a gap in which a track found no pair is registered from what the other gaps predict -- the nearest "
                         "unmatched source cluster, the track's destination cluster, the predicted translation -- and an accepted pair is appended "
                         "to that gap's pair rows and transforms (flow, objects and tracks of that gap follow); after --tracks-repair when both are "
                         "given; not with --tracks-log, not with --protocol reference")
    ap.add_argument("--tracks-log", nargs="?", const=True, default=None, metavar="FILE",
                    help="object tracks over a log: the directory's frame-pair files are consecutive (file k registers sweep k onto "
                         "sweep k + 1; the source of a file is the destination of the one before, carried over by the file's pose); "
                         "track ids are carried from file to file by nearest rows, per track a path, a mean velocity and whether "
                         "its velocity changes smoothly (FILE: one JSON line per track); uses --sweep-seconds, --objects-min-speed "
                         "and --tracks-min-iou; one process only; not with --protocol reference; not for sequence files")
    ap.add_argument("--tracks-log-radius", type=float, default=utils_tracks.CARRY_RADIUS, metavar="R",
                    help="with --tracks-log: a row takes the id of the nearest row of the other view within R metres")
    ap.add_argument("--tracks-log-min-share", type=float, default=utils_tracks.CARRY_MIN_SHARE, metavar="Q",
                    help="with --tracks-log: when fewer than Q of a file's source rows find a row of the file before, the ids start afresh")
    ap.add_argument("--tracks-log-max-dv", type=float, default=utils_tracks.MAX_DV, metavar="V",
                    help="with --tracks-log: a track is smooth when its velocity changes by at most V m/s between adjacent files")
    ap.add_argument("--save-metrics", metavar="FILE", default=None,
                    help="--protocol reference: write the meters' per-sequence values as the reference's closing file (main.py:298-312)")
    return ap


def main(argv=None):
    ns = argument_parser().parse_args(argv)
    if ns.class_table and not (ns.protocol == "reference" and ns.dataset == "argo"):
        raise SystemExit("--class-table goes with --protocol reference --dataset argo (the category names are Argoverse 2's)")
    if ns.bucketed_epe and not (ns.protocol == "reference" and ns.dataset == "argo"):
        raise SystemExit("--bucketed-epe goes with --protocol reference --dataset argo (the classes and the buckets are Argoverse 2's)")
    if ns.residual is not None and ns.protocol == "reference":
        raise SystemExit("--residual is not built into --protocol reference (COVERAGE.md row 13): run the frame pairs without --protocol")
    if ns.residual_segments is not None and ns.residual is None:
        raise SystemExit("--residual-segments goes with --residual (the two share the radius)")
    if ns.residual_sight is not None and ns.residual_segments is None:
        raise SystemExit("--residual-sight goes with --residual-segments (it judges the segments that one lists)")
    if ns.residual_sight is not None and len(ns.residual_sight) not in (0, 3):
        raise SystemExit("--residual-sight takes no number or the origin's three: X Y Z")
    if ns.residual_trust and ns.residual_segments is None:
        raise SystemExit("--residual-trust goes with --residual --residual-segments (it spreads their verdicts over the rows)")
    if ns.objects is not None and ns.protocol == "reference":
        raise SystemExit("--objects is not built into --protocol reference (COVERAGE.md row 17): run the frame pairs without --protocol")
    if ns.objects is not None and not (ns.sweep_seconds > 0 and ns.objects_min_speed >= 0):
        raise SystemExit("--sweep-seconds must be positive and --objects-min-speed must not be negative")
    if ns.tracks_repair and ns.tracks is None:
        raise SystemExit("--tracks-repair goes with --tracks (it registers again the gaps the tracks name; --tracks-log has no repair)")
    if ns.tracks_fill and ns.tracks is None:
        raise SystemExit("--tracks-fill goes with --tracks (it fills the gaps the tracks name; --tracks-log has no fill)")
    if ns.tracks_fill and ns.tracks_log is not None:
        raise SystemExit("--tracks-fill is not built into --tracks-log: a log's files share no sweep whose other gaps could predict the missing one")
    if ns.tracks is not None and ns.protocol == "reference":
        raise SystemExit("--tracks is not built into --protocol reference (COVERAGE.md row 18): run the frame pairs without --protocol")
    if ns.tracks is not None and not (ns.sweep_seconds > 0 and ns.objects_min_speed >= 0 and 0 < ns.tracks_min_iou <= 1 and ns.tracks_max_residual >= 0):
        raise SystemExit("--sweep-seconds must be positive, --objects-min-speed and --tracks-max-residual must not be negative, "
                         "--tracks-min-iou must lie in (0, 1]")
    if ns.tracks_log is not None and ns.protocol == "reference":
        raise SystemExit("--tracks-log is not built into --protocol reference (COVERAGE.md row 19): run the frame pairs without --protocol")
    if ns.tracks_log is not None and not (ns.sweep_seconds > 0 and ns.objects_min_speed >= 0 and 0 < ns.tracks_min_iou <= 1 and
                                          1e-3 <= ns.tracks_log_radius <= 1e3 and 0 <= ns.tracks_log_min_share <= 1 and ns.tracks_log_max_dv >= 0):
        raise SystemExit("--sweep-seconds must be positive, --objects-min-speed and --tracks-log-max-dv must not be negative, --tracks-min-iou "
                         "must lie in (0, 1], --tracks-log-radius in [1e-3, 1e3] metres, --tracks-log-min-share in [0, 1]")
    if ns.tracks_log is not None and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--tracks-log under more than one rank: a log's files would have to meet on one rank in their order, which is not built")
    if ns.tracks_log is not None and any(is_sequence(p) for p in list_frame_pairs(ns.directory)):
        raise SystemExit("--tracks-log takes frame-pair files: which sweep consecutive multi-frame samples share is not in a sequence file "
                         "(utils_tracks.TrackState(track_of_row=...) composes that case)")
    if ns.save_trust is not None and not ns.save_flows:
        raise SystemExit("--save-trust goes with --save-flows (the bytes go into the saved flow's file)")
    if ns.save_trust is not None and len(ns.save_trust) not in (0, 3):
        raise SystemExit("--save-trust takes no number or the origin's three: X Y Z")
    if (ns.save_flows or ns.save_metrics) and ns.protocol != "reference":
        raise SystemExit("--save-flows and --save-metrics go with --protocol reference")
    if ns.dataset == "argo":
        if ns.num_frames not in (None, 2):
            raise SystemExit(f"--dataset argo: an Argoverse 2 sample has two frames (--num-frames {ns.num_frames})")
        if ns.protocol != "reference":
            raise SystemExit("--dataset argo goes with --protocol reference (without it every file is a plain frame pair already)")
    num_frames = ns.num_frames if ns.num_frames is not None else 2 if ns.dataset == "argo" else 5
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    args = SimpleNamespace(**{k: getattr(ns, k) for k in DEFAULT_ARGS})
    args.max_points, args.min_cluster_size, args.chunk_size = int(args.max_points), int(args.min_cluster_size), int(args.chunk_size)
    args.num_clusters = int(args.num_clusters)
    args.pose_source, args.save_poses = ns.pose_source, ns.save_poses
    if ns.native_cluster:
        args.native_cluster = True
    if ns.ego_deskew or ns.ego_fixed_threshold:
        args.ego_motion = dict(deskew=ns.ego_deskew, fixed_threshold=ns.ego_fixed_threshold)
    if ns.protocol == "reference":
        if world > 1 and (ns.if_verbose or ns.report):
            raise SystemExit("--if-verbose / --report under more than one rank: merging the reports is not built")
        if args.range_x is None or args.range_y is None:
            args.range_x, args.range_y = 32.0, 32.0                                    # main.py:69-72
        args.num_frames, args.range_z, args.ground_slack, args.eval_ground = num_frames, ns.range_z, ns.ground_slack, ns.eval_ground
        args.ground = ns.ground
        if ns.if_verbose or ns.report:
            args.if_verbose = True
        if ns.class_table:
            args.class_table = ns.class_table
        if ns.bucketed_epe:
            args.bucket_table = True
        if ns.save_flows:
            args.save_flows = True
        if ns.save_trust is not None:
            args.save_trust = tuple(ns.save_trust) if ns.save_trust else True
        shard = dict(rank=rank, world=world) if world > 1 else {}
        if ns.dataset == "argo":
            res = run_sequences(args, [p for p in list_frame_pairs(ns.directory) if is_argo(p)], device, in_flight=ns.in_flight, dataset="argo", **shard)
        else:
            res = run_sequences(args, [p for p in list_frame_pairs(ns.directory) if is_sequence(p)], device, in_flight=ns.in_flight, **shard)
        if rank == 0:
            reports = res.pop("segments", None)
            if ns.report:
                with open(ns.report, "w") as f:
                    json.dump(worst_segments(reports, ns.report_epe), f, indent=1)
            metrics = res.pop("metrics")
            print(utils_eval.format_metric_table(metrics, args.num_frames))
            if ns.save_metrics:
                utils_eval.save_metrics_file(ns.save_metrics, metrics, args.num_frames)
            if ns.class_table:
                table = res.pop("class_table")
                print(utils_eval.format_class_table(table, fine=ns.class_table == "fine"))
                shown = table if ns.class_table == "fine" else table.meta(utils_eval.ARGO_META_GROUPS)
                res["class_table"] = dict(rows=list(shown.names or utils_eval.ARGO_ROW_NAMES), counts=shown.counts.tolist(),
                                          esum=shown.esum.tolist(), ssum=shown.ssum.tolist())
            if ns.bucketed_epe:
                res.pop("bucket_table")
                print(utils_eval.format_bucketed_epe(res["bucketed_epe"]))
            print(json.dumps(res))
        if world > 1:
            dist.destroy_process_group()
        return
    if ns.residual is not None:
        args.residual = ns.residual
    if ns.residual_segments is not None:
        if world > 1:
            raise SystemExit("--residual-segments under more than one rank: merging the lists is not built")
        args.residual_segments = ns.residual_segments
    if ns.residual_sight is not None:
        args.residual_sight = tuple(ns.residual_sight) if ns.residual_sight else True
    if ns.residual_trust:
        args.residual_trust = True
    if ns.objects is not None:
        if world > 1:
            raise SystemExit("--objects under more than one rank: merging the files is not built")
        args.objects, args.sweep_seconds, args.objects_min_speed = ns.objects, ns.sweep_seconds, ns.objects_min_speed
    if ns.tracks is not None:
        if world > 1:
            raise SystemExit("--tracks under more than one rank: a sample's gaps would have to meet on one rank, which is not built")
        args.tracks, args.sweep_seconds, args.objects_min_speed = ns.tracks, ns.sweep_seconds, ns.objects_min_speed
        args.tracks_min_iou, args.tracks_max_residual = ns.tracks_min_iou, ns.tracks_max_residual
        if ns.tracks_repair:
            args.tracks_repair = True
        if ns.tracks_fill:
            args.tracks_fill = True
    if ns.tracks_log is not None:
        args.tracks_log, args.sweep_seconds, args.objects_min_speed, args.tracks_min_iou = ns.tracks_log, ns.sweep_seconds, ns.objects_min_speed, ns.tracks_min_iou
        args.tracks_log_radius, args.tracks_log_min_share, args.tracks_log_max_dv = ns.tracks_log_radius, ns.tracks_log_min_share, ns.tracks_log_max_dv
    summary = run_stream(args, list_frame_pairs(ns.directory), device, rank, world, ns.repeat, in_flight=ns.in_flight)
    if rank == 0:
        if ns.residual is not None:
            print(utils_eval.format_residual(*residual_tables(summary["residual"])))
        if ns.residual_segments is not None:
            lines = utils_eval.format_segment_sight if ns.residual_sight is not None else utils_eval.format_segment_residual
            print("\n".join(lines(summary["residual_segments"]["worst"])))
        print(json.dumps(summary))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""The frame pair itself: the data class, its .npz file and its arrays on the device.  A leaf module -- the loaders of whole
sequences, the registration paths and the drivers (frame_pairs.py) and the judges of a registered frame pair (pair_judges.py)
build on it; frame_pairs.py's docstring describes the file format."""
import os

import numpy as np
import torch


class FramePair:
    def __init__(self, points_src, points_dst, labels_src=None, labels_dst=None, pose=None, gt_flow=None, mask=None,
                 name="", nonground_src=None, nonground_dst=None, gap=1, points_src_raw=None, pose_source="given", sequence=None):
        self.points_src = np.ascontiguousarray(points_src, dtype=np.float32)[:, 0:3]
        self.points_dst = np.ascontiguousarray(points_dst, dtype=np.float32)[:, 0:3]
        if (labels_src is None) != (labels_dst is None):
            raise ValueError(f"frame pair {name!r}: labels of both clouds or of neither")
        self.labels_src = None if labels_src is None else np.ascontiguousarray(labels_src, dtype=np.float32)
        self.labels_dst = None if labels_dst is None else np.ascontiguousarray(labels_dst, dtype=np.float32)
        self.nonground_src = None if nonground_src is None else np.asarray(nonground_src).astype(bool)
        self.nonground_dst = None if nonground_dst is None else np.asarray(nonground_dst).astype(bool)
        for m, pts in ((self.nonground_src, self.points_src), (self.nonground_dst, self.points_dst)):
            if m is not None and m.shape != (len(pts),):
                raise ValueError(f"frame pair {name!r}: one non-ground flag per point required")
        if self.labels_src is not None and (
                len(self.labels_src) != len(self.points_src) or len(self.labels_dst) != len(self.points_dst)):
            raise ValueError(f"frame pair {name!r}: one label per point required "
                             f"({len(self.labels_src)}/{len(self.points_src)} src, "
                             f"{len(self.labels_dst)}/{len(self.points_dst)} dst)")
        self.pose = np.eye(4, dtype=np.float32) if pose is None else np.asarray(pose, dtype=np.float32).reshape(4, 4)
        # the pose as given (the reference's ego poses are float64 and main.py:200 takes their norm as such)
        self.pose_exact = np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64).reshape(4, 4)
        self.gt_flow = None if gt_flow is None else np.asarray(gt_flow, dtype=np.float32)
        if self.gt_flow is not None and self.gt_flow.shape != self.points_src.shape:
            raise ValueError(f"frame pair {name!r}: gt_flow must be [Ns,3]")
        self.mask = None if mask is None else np.asarray(mask)
        self.name = name
        self.pose_source = pose_source        # where the ego pose came from (load_sequence), reported by run_stream
        # multi-gap samples (Waymo / nuScenes): frame `gap` against frame 0; the flow is reported on the source
        # points BEFORE ego-motion compensation (main.py:230-234), registration runs on the compensated ones
        self.gap = int(gap)
        # the sample this frame pair is one gap of (load_sequence: the file's path), or None: the frame pairs of one sample share
        # points_dst row for row, which is what run_stream's object tracks link (utils_tracks)
        self.sequence = sequence
        self.points_src_raw = None if points_src_raw is None else np.ascontiguousarray(points_src_raw, dtype=np.float32)[:, 0:3]
        if self.points_src_raw is not None and self.points_src_raw.shape != self.points_src.shape:
            raise ValueError(f"frame pair {name!r}: points_src_raw must match points_src")


def save_frame_pair(path, fp):
    arrays = dict(points_src=fp.points_src, points_dst=fp.points_dst, pose=fp.pose)
    for k in ("labels_src", "labels_dst", "nonground_src", "nonground_dst"):
        if getattr(fp, k) is not None:
            arrays[k] = getattr(fp, k)
    if fp.gt_flow is not None:
        arrays["gt_flow"] = fp.gt_flow
    if fp.mask is not None:
        arrays["mask"] = fp.mask
    np.savez_compressed(path, **arrays)


def load_frame_pair(path):
    with np.load(path) as z:
        keys = set(z.files)

        def first(*names):
            for n in names:
                if n in keys:
                    return z[n]
            return None

        labels_src, labels_dst = first("labels_src", "label_src"), first("labels_dst", "label_dst")
        ng = dict(nonground_src=first("nonground_src"), nonground_dst=first("nonground_dst"))
        if "points_src" in keys:
            return FramePair(z["points_src"], z["points_dst"], labels_src, labels_dst, first("pose"),
                             first("gt_flow"), first("mask"), name=os.path.basename(path), **ng)
        if "pc1" in keys:                                   # dataset_argo.py:34-53, demo.py:37-51
            v0, v1 = z["pc1_flows_valid_idx"], z["pc2_flows_valid_idx"]
            gt = z["gt_flow_0_1"][v0] if "gt_flow_0_1" in keys else None
            return FramePair(z["pc1"][v0], z["pc2"][v1], labels_src, labels_dst, first("pose"), gt, first("mask"),
                             name=os.path.basename(path), **ng)
        raise ValueError(f"{path}: neither points_src/points_dst nor pc1/pc2 present")


def make_resident(fp, device):
    """Upload the frame pair's arrays once and keep the device tensors with it (`register_frame_pair_native` then takes those:
    inputs resident in HBM, what bench.py's stream workload times).  -> fp"""
    device = torch.device(device)
    keep = {}
    for name in ("points_src", "points_dst", "labels_src", "labels_dst", "points_src_raw"):
        arr = getattr(fp, name)
        if arr is not None:
            keep[name] = torch.from_numpy(arr).to(device)
    fp._resident = (device, keep)
    return fp


def _input(fp, name, device):
    res = getattr(fp, "_resident", None)
    if res is not None and res[0] == torch.device(device) and name in res[1]:
        return res[1][name]
    return _upload(getattr(fp, name), device)


def _upload(arr, device):
    """Host array -> device tensor, from pageable memory.  (Measured on this stack: 41 us for a 63 k-point cloud; the
    same upload through a pinned staging buffer with a non-blocking copy made a stream of frame pairs ten times SLOWER --
    the copies serialise against the kernels of the other streams.)"""
    return torch.from_numpy(arr).to(device)

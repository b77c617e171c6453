"""Drop-in for the reference's utils_debug.debug_frame (utils_debug.py:22-93): the numbers of its three lines per frame and,
under args.if_verbose, the per-segment evaluation it calls.  Nothing is visualised."""
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, utils_eval, utils_flow

FRAME_CLASSES = ("overall", "static", "dynamic")


def frame_rows(args, src, sd_label, fb_label, flow_gt, flow):
    """utils_debug.py:37-61: compute_epe_test over all rows, the rows with sd_label == 0 and those with sd_label == 1, after
    the z crop unless args.eval_ground -- through icpflow_seq_metrics with two frames (every row in gap 1) and infinite x and y
    ranges.  -> {class: (EPE float64, four float32 fractions, number of rows)}; `dynamic` is absent when it has no row
    (utils_debug.py:59), `static` is NaN then, as the reference's mean of nothing."""
    _lib.require_gpu(src, sd_label, fb_label, flow_gt, flow)
    n = len(src)
    a = SimpleNamespace(num_frames=2, eval_ground=bool(getattr(args, "eval_ground", False)), range_x=float("inf"), range_y=float("inf"),
                        range_z=float(getattr(args, "range_z", 0.0)), ground_slack=float(getattr(args, "ground_slack", 0.0)))
    fb = sd_label if fb_label is None else fb_label
    data = dict(raw_points=src, time_indice=torch.ones(n, dtype=torch.int32, device=src.device), sd_labels=sd_label, fb_labels=fb,
                scene_flow=flow_gt)
    table, esum, _, _ = utils_eval.sequence_table(a, data, flow)
    out = {}
    with np.errstate(all="ignore"):
        for name, c in (("overall", 0), ("static", 1), ("dynamic", 4)):
            if name == "dynamic" and int(table[1, c, 0]) == 0:
                continue
            out[name] = utils_eval._cell_metrics(table, esum, 1, c) + (int(table[1, c, 0]),)
    return out


def frame_lines(args, j, rows):
    """the reference's three lines (utils_debug.py:50, 55, 61), the width of the class name as it writes them"""
    label = {"overall": " overall", "static": " static", "dynamic": "dynamic"}
    return [f"debug frame: {j}/{args.num_frames}, {label[k]}, EPE: {v[0]:.4f}, ACC3DS: {v[1]:.4f}, ACC3DR: {v[2]:.4f}, "
            f"Outlier: {v[3]:.4f}, Routlier: {v[4]:.4f}" for k, v in rows.items()]


def debug_frame(args, result):
    """utils_debug.py:22-93 on the reference's `result` dict (j, src, dst, pose, sd_label, fb_label, scene_flow, src_label,
    dst_label, flow, and for the segments transformations and pairs) of GPU tensors: prints the three per-frame lines and
    returns dict(frame = frame_rows(...), lines, segments = flow_evaluation's report under args.if_verbose, else None)."""
    j = result["j"]
    src = result["src"]
    rows = frame_rows(args, src, result["sd_label"], result.get("fb_label"), result["scene_flow"], result["flow"])
    lines = frame_lines(args, j, rows)
    for line in lines:
        print(line)
    segments = None
    if getattr(args, "if_verbose", False):
        z_min = None if getattr(args, "eval_ground", False) else args.range_z + args.ground_slack
        segments = utils_flow.flow_evaluation(src, result["dst"], result["src_label"], result["dst_label"], result["flow"],
                                              result["scene_flow"], result["pose"], result["transformations"], pairs=result["pairs"],
                                              z_min=z_min, verbose=True)
    return dict(frame=rows, lines=lines, segments=segments)

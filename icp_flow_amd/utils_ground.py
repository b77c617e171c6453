"""Drop-in for the reference's ground removal (utils_ground.py:16-66): the height threshold, Patchwork++ with the
reference's fixed parameters, and their AND.

The Patchwork++ half runs on the GPU (icpflow_ground_segment, csrc/ground.hip): a restatement of the method in fp64 -- the
package itself needs Eigen and is not built here (COVERAGE.md, named deviations).  There is no CPU path."""
import ctypes

import numpy as np
import torch


def segment_ground_thres(args, points):
    """True = non-ground: z > range_z + ground_slack (utils_ground.py:27-30).  numpy or torch in, same out."""
    thr = args.range_z + args.ground_slack
    if isinstance(points, torch.Tensor):
        return ~(points[:, 2] <= thr)
    return ~(np.asarray(points)[:, 2] <= thr)


def segment_ground_pypatchworkpp(points, return_table=False):
    """True = non-ground by Patchwork++ (utils_ground.py:43-66).  points [n, >= 3], cast to float32 as pybind casts them for
    the reference.  numpy in gives numpy out; a GPU tensor in gives a GPU tensor out, resident.  return_table: also the
    per-patch table, float64 [504, 16] (include/icpflow_hip.h)."""
    from . import _lib
    as_numpy = not isinstance(points, torch.Tensor)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("icp_flow_amd: segment_ground_pypatchworkpp needs a GPU (HIP) device -- there is no CPU path")
        points = torch.from_numpy(np.ascontiguousarray(np.asarray(points)[:, 0:3].astype(np.float32))).cuda()
    _lib.require_gpu(points)
    if points.dim() != 2 or points.shape[1] < 3:
        raise RuntimeError(f"points: expected shape [n, >= 3], got {tuple(points.shape)}")
    pts = points[:, 0:3].to(torch.float32).contiguous()
    n, dev = int(pts.shape[0]), pts.device
    par = _lib.GroundParams.defaults()
    labels = torch.empty(n, dtype=torch.uint8, device=dev)
    table = torch.zeros((_lib.GROUND_PATCHES, _lib.GROUND_TABLE_COLS), dtype=torch.float64, device=dev) if return_table else None
    if n > 0:
        need = int(_lib._L.icpflow_ground_workspace_bytes(n, ctypes.byref(par)))
        with torch.cuda.device(dev):
            ws = _lib.workspace(dev, need)
            _lib.call("icpflow_ground_segment", _lib.ptr(pts), 3, n, ctypes.byref(par), _lib.ptr(labels), _lib.ptr(table), _lib.ptr(ws),
                      ctypes.c_size_t(ws.numel()), _lib.stream(dev))
    out = labels.bool()
    if as_numpy:
        out = out.cpu().numpy()
        table = None if table is None else table.cpu().numpy()
    return (out, table) if return_table else out


def segment_ground(args, points):
    """True = non-ground: the threshold AND Patchwork++ (utils_ground.py:16-23)."""
    patch = segment_ground_pypatchworkpp(points)
    return segment_ground_thres(args, points) & patch

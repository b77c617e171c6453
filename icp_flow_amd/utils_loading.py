"""Drop-in for the pose arithmetic of the reference's loader (utils_loading.py:21-48): the two functions that turn a
Waymo / nuScenes sample's poses into its ground-truth scene flow (dataset_pca.py:66-69), computed by icpflow_seq_gt_flow
(csrc/seqeval.hip) in fp64.  numpy arrays or device tensors in, the same kind out; there is no CPU path.

Where this differs from numpy on purpose: a time index outside [0, n_frames) or an instance label outside [0, M) raises
(numpy wraps a negative index around to the last pose, and checks only the combination inst * n_frames + t)."""
import ctypes

import numpy as np
import torch

from . import _lib


def _device_for(*arrays):
    """The device of the first device tensor among the arguments; for numpy input the current GPU."""
    for a in arrays:
        if isinstance(a, torch.Tensor):
            _lib.require_gpu(a)
            return a.device
    if not torch.cuda.is_available():
        _lib.require_gpu(arrays[0])          # (raises the package's message: there is no CPU path)
    return torch.device("cuda", torch.cuda.current_device())


def to_device(a, dtype, device):
    """numpy array or tensor -> contiguous device tensor of `dtype` (widening float32 -> float64 is exact)."""
    if isinstance(a, torch.Tensor):
        _lib.require_gpu(a)
        return a.to(device=device, dtype=dtype).contiguous()
    a = np.asarray(a)
    if a.dtype == object:
        raise TypeError("an object array cannot be evaluated on the device")
    return torch.from_numpy(np.ascontiguousarray(a)).to(device).to(dtype).contiguous()


def _like(out, template):
    return out if isinstance(template, torch.Tensor) else out.cpu().numpy()


def seq_transform(points, time_indice, inst_labels, ego, inst_tsfm, output):
    """icpflow_seq_gt_flow on numpy arrays or device tensors -> float64 device tensor [m,3]; raises on rows it refused."""
    device = _device_for(points, time_indice, inst_labels, ego, inst_tsfm)
    pts = to_device(points, torch.float64, device)
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError(f"points: expected [m, >=3], got {tuple(pts.shape)}")
    pts = pts[:, 0:3].contiguous()
    m = pts.shape[0]
    tim = to_device(time_indice, torch.int32, device)
    if tim.shape != (m,):
        raise ValueError("time_indice: one entry per point required")
    F = K = 0
    ego_d = tsfm_d = inst = None
    if ego is not None:
        ego_d = to_device(ego, torch.float64, device)
        if ego_d.dim() != 3 or ego_d.shape[1:] != (4, 4):
            raise ValueError(f"tsfm: expected [n_frames,4,4], got {tuple(ego_d.shape)}")
        F = ego_d.shape[0]
    if inst_tsfm is not None:
        tsfm_d = to_device(inst_tsfm, torch.float64, device)
        if tsfm_d.dim() != 4 or tsfm_d.shape[2:] != (4, 4) or (F and tsfm_d.shape[1] != F):
            raise ValueError(f"tsfm: expected [M,n_frames,4,4], got {tuple(tsfm_d.shape)}")
        K, F = tsfm_d.shape[0], tsfm_d.shape[1]
        inst = to_device(inst_labels, torch.int32, device)
        if inst.shape != (m,):
            raise ValueError("inst_labels: one entry per point required")
    out = torch.empty((m, 3), dtype=torch.float64, device=device)
    bad = torch.empty(1, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_seq_gt_flow_workspace_bytes(m))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_seq_gt_flow", _lib.ptr(pts), _lib.ptr(tim), _lib.ptr(inst), m, _lib.ptr(ego_d), F, _lib.ptr(tsfm_d), K,
                  int(output), _lib.ptr(out), _lib.ptr(bad), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    n_bad = int(bad.item())
    if n_bad:
        raise IndexError(f"{n_bad} of {m} points have a time index outside [0, {F})" +
                         (f" or an instance label outside [0, {K})" if tsfm_d is not None else "") +
                         " (numpy's negative-index wrap-around is not reproduced)")
    return out


def ego_motion_compensation(points, time_indice, tsfm):
    """utils_loading.py:21-31: points [N,3], time_indice [N], tsfm [n_frames,4,4] -> tsfm[time] applied to every point, float64."""
    return _like(seq_transform(points, time_indice, None, tsfm, None, _lib.SEQ_OUT_POINTS), points)


def reconstruct_sequence(points, time_indice, inst_labels, tsfm, n_frames):
    """utils_loading.py:33-48: points [N,3], time_indice [N], inst_labels [N], tsfm [M,n_frames,4,4] ->
    tsfm[inst, time] applied to every point, float64."""
    assert n_frames == tsfm.shape[1]
    return _like(seq_transform(points, time_indice, inst_labels, None, tsfm, _lib.SEQ_OUT_POINTS), points)


def scene_flow(raw_points, time_indice, inst_labels, ego_motion_gt, inst_motion_gt):
    """dataset_pca.py:66-69 in one launch: reconstruct_sequence(ego_motion_compensation(raw)) - raw, float64 [m,3]."""
    return _like(seq_transform(raw_points, time_indice, inst_labels, ego_motion_gt, inst_motion_gt, _lib.SEQ_OUT_FLOW), raw_points)

"""Drop-in for the pose arithmetic of the reference's loader (utils_loading.py:21-48): the two functions that turn a
Waymo / nuScenes sample's poses into its ground-truth scene flow (dataset_pca.py:66-69), computed by icpflow_seq_gt_flow
(csrc/seqeval.hip) in fp64.  numpy arrays or device tensors in, the same kind out; there is no CPU path.
`argo_sample` is the front of the other loader, dataset_argo.py:47-50, 66-71, 83-89 (icpflow_seq_argo_sample): the two-frame
sample of an Argoverse 2 file with its static / dynamic and foreground / background labels, built on the device.

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
    from . import utils_eval
    tim = utils_eval._time_indices(time_indice, F, device)      # a value that equals no integer of [0, F) is -1: refused below
    if tim.shape != (m,):
        raise ValueError("time_indice: one entry per point required")
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


# dataset_argo.py:23-25: the reference looks its six background categories up by POSITION in its id table sorted by id, and
# that table starts at id -1 -- so these are the categories' ids + 1 (ids 4, 7, 8, 12, 20, 21), compared with the file's classes
ARGO_BACKGROUND_IDXES = (5, 8, 9, 13, 21, 22)
ARGO_DYNAMIC_THRESHOLD = 0.5 * 0.1            # dataset_argo.py:66-67: 10 Hz, more than 0.5 m/s is dynamic


def _file_dtype(a, name):
    """The type a file stores an array in -> (torch dtype, numpy type, ICPFLOW_DTYPE_*)"""
    kind = str(a.dtype).replace("torch.", "")
    if kind == "float32":
        return torch.float32, np.float32, _lib.DTYPE_FLOAT32
    if kind == "float64":
        return torch.float64, np.float64, _lib.DTYPE_FLOAT64
    raise TypeError(f"{name}: float32 or float64 expected, got {a.dtype}")


def argo_sample(pc1, pc2, flow_0_1, classes1, valid1, valid2, background=None, device=None):
    """dataset_argo.py:47-50, 66-71, 83-89 on the device (icpflow_seq_argo_sample): the arrays of one Argoverse 2 file --
    pc1 [n1,3], pc2 [n2,3], gt_flow_0_1 [n1,3], pc1_classes [n1], the two *_flows_valid_idx (index lists, or boolean masks:
    np.flatnonzero on the host first) -- as numpy arrays or device tensors -> the sample calculate_metrics reads, a dict of
    device tensors of m = m2 + m1 rows, frame 0 (pc2's rows) first: raw_points (in the points' own dtype: the kernel's
    float64 rows narrowed back, which is exact, so that the evaluation rounds its crop thresholds as numpy does for that
    dtype), time_indice, sd_labels, fb_labels (int32), scene_flow (float64), classes (float64: pc1_classes of frame 1's rows, NaN
    for frame 0's -- what utils_eval.class_table reads).  `background`: the class values that are not
    foreground besides -1 (default ARGO_BACKGROUND_IDXES).  An index outside [0, n) raises IndexError (numpy's negative
    wrap-around is not reproduced).  There is no CPU path."""
    if device is None:
        device = _device_for(pc1, pc2, flow_0_1, classes1)
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("icp_flow_amd: an Argoverse 2 sample is built on the GPU -- there is no CPU path")
    p_t, _, p_code = _file_dtype(pc1, "pc1")
    if _file_dtype(pc2, "pc2")[0] != p_t:
        raise TypeError("pc1 and pc2 must be stored in one dtype")
    f_t, f_np, f_code = _file_dtype(flow_0_1, "gt_flow_0_1")
    p1, p2 = to_device(pc1, p_t, device), to_device(pc2, p_t, device)
    flow = to_device(flow_0_1, f_t, device)
    for name, a in (("pc1", p1), ("pc2", p2), ("gt_flow_0_1", flow)):
        if a.dim() != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: expected [n,3], got {tuple(a.shape)}")
    n1, n2 = p1.shape[0], p2.shape[0]
    cls = to_device(classes1, torch.float64, device)
    if flow.shape[0] != n1 or cls.shape != (n1,):
        raise ValueError("gt_flow_0_1 and pc1_classes: one row per point of pc1 required")

    def index_list(v, n, name):
        if (isinstance(v, torch.Tensor) and v.dtype == torch.bool) or (not isinstance(v, torch.Tensor) and np.asarray(v).dtype == bool):
            host = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if host.shape != (n,):
                raise IndexError(f"{name}: a boolean mask of {host.shape} for {n} points")
            v = np.flatnonzero(host)
        v = to_device(v, torch.int64, device)
        if v.dim() != 1:
            raise ValueError(f"{name}: a list of indices expected, got {tuple(v.shape)}")
        return v

    v1, v2 = index_list(valid1, n1, "pc1_flows_valid_idx"), index_list(valid2, n2, "pc2_flows_valid_idx")
    m1, m2 = v1.shape[0], v2.shape[0]
    m = m1 + m2
    bg = np.ascontiguousarray(ARGO_BACKGROUND_IDXES if background is None else background, dtype=np.int32).reshape(-1)
    pts = torch.empty((m, 3), dtype=torch.float64, device=device)
    tim, sd, fb = (torch.empty(m, dtype=torch.int32, device=device) for _ in range(3))
    out_flow = torch.empty((m, 3), dtype=torch.float64, device=device)
    bad = torch.empty(1, dtype=torch.int64, device=device)
    # the threshold as numpy compares it with a norm of the flow's dtype (utils_eval._threshold_for's idea)
    threshold = float(np.asarray(ARGO_DYNAMIC_THRESHOLD, dtype=np.float64).astype(f_np))
    with torch.cuda.device(device):
        _lib.call("icpflow_seq_argo_sample", _lib.ptr(p1), n1, _lib.ptr(p2), n2, p_code, _lib.ptr(flow), f_code, _lib.ptr(cls),
                  _lib.ptr(v1), m1, _lib.ptr(v2), m2, bg.ctypes.data_as(ctypes.c_void_p), len(bg), threshold, _lib.ptr(pts),
                  _lib.ptr(tim), _lib.ptr(sd), _lib.ptr(fb), _lib.ptr(out_flow), _lib.ptr(bad), _lib.stream(device))
    n_bad = int(bad.item())
    if n_bad:
        raise IndexError(f"{n_bad} of {m} valid indices lie outside their cloud ([0, {n1}) for pc1, [0, {n2}) for pc2; "
                         "numpy's negative-index wrap-around is not reproduced)")
    # the class of every row for utils_eval.class_table: NaN for frame 0, whose rows are never counted (the indices are known good here)
    classes = torch.cat([torch.full((m2,), float("nan"), dtype=torch.float64, device=device), cls.index_select(0, v1)])
    return dict(raw_points=pts.to(p_t), time_indice=tim, sd_labels=sd, fb_labels=fb, scene_flow=out_flow, classes=classes)

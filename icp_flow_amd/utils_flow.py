"""Drop-in for the reference's utils_flow.flow_estimation_torch (utils_flow.py:57-69) and its per-segment evaluation
flow_evaluation (utils_flow.py:72-150; numbers and text, nothing is visualised)."""
import numpy as np
import torch

from . import _lib


def flow_estimation_torch(args, src_points, dst_points, src_labels, dst_labels, pairs, transformations, pose):
    """Per-point flow: points of a matched cluster move with T_cluster @ pose, all others with
    pose alone; flow = moved - point.  The reference builds an N x P label-equality matrix and two
    N-batched 4x4 bmm; here one thread per point looks its label up and applies one 3x4 map."""
    assert len(src_points) == len(src_labels)
    pts = src_points[:, 0:3].contiguous().float()
    _lib.require_gpu(pts, src_labels)
    dev = pts.device
    N = pts.shape[0]
    P = int(pairs.shape[0])
    lab = src_labels.contiguous().float()
    flow = torch.empty((N, 3), dtype=torch.float32, device=dev)
    if P:
        # the matched source labels are read in place: column 0 of the float32 pair rows (no slice kernel)
        rows = pairs if (pairs.device == dev and pairs.dtype == torch.float32 and pairs.dim() == 2 and pairs.stride(1) == 1
                         and 1 <= pairs.stride(0) <= 1024) else pairs[:, 0:1].to(dev).contiguous().float()
        stride = int(rows.stride(0)) if rows.shape[1] > 1 else 1
        T = transformations.to(dev).contiguous().float()
    else:
        rows, stride, T = None, 1, None
    pose = pose.to(dev).contiguous().float()
    _lib.call("icpflow_flow_rigid_rows", _lib.ptr(pts), _lib.ptr(lab), N, _lib.ptr(rows), stride, _lib.ptr(T), P,
              _lib.ptr(pose), _lib.ptr(flow), _lib.stream(dev))
    return flow


# ---- the per-segment evaluation of the reference's verbose loop (utils_flow.py:72-150) ------------------------------------
SEGMENT_FIELDS = ("label", "rows", "n", "sum_e", "epe", "accs", "accr", "outlier", "routlier", "len_j", "mean_i", "mean_j", "pair_index",
                  "matched_dst", "translation", "rotation_zyx_deg")
LARGE_EPE = 2.0          # utils_flow.py:112


class SegmentReport:
    """One row per source segment (distinct source label, ascending), numpy arrays: label, rows (of the segment), n (kept rows:
    the reference's len_i after debug_frame's crop), sum_e (the kernel's sum of the end point error), epe (float64, sum_e / n), accs / accr / outlier / routlier (float32 means, as
    compute_epe_test returns them), len_j and mean_j [S,3] (the destination rows of the same label, uncropped), mean_i [S,3],
    pair_index and matched_dst (from pairs[:, 0:2], or -1), translation (|mean(x + flow) - mean(x)|) and rotation_zyx_deg [S,3]
    (of the matched transform, NaN without one).  `lines` is the text `verbose=True` printed."""

    def __init__(self, **arrays):
        for k in SEGMENT_FIELDS:
            setattr(self, k, arrays[k])
        self.lines = arrays.get("lines", [])
        self.moved = arrays.get("moved")          # mean(x + flow) [S,3], behind `translation`

    def __len__(self):
        return len(self.label)

    def worst(self, threshold=LARGE_EPE):
        """-> [dict] of the segments with epe > threshold, worst first (a NaN epe is not above any threshold)"""
        with np.errstate(invalid="ignore"):
            idx = np.flatnonzero(self.epe > threshold)
        idx = idx[np.argsort(-self.epe[idx], kind="stable")]
        return [dict(label=float(self.label[k]), n=int(self.n[k]), epe=float(self.epe[k]),
                     matched_label=float(self.matched_dst[k]) if self.pair_index[k] >= 0 else None, translation=float(self.translation[k]),
                     rotation_zyx_deg=[float(v) for v in self.rotation_zyx_deg[k]] if self.pair_index[k] >= 0 else None) for k in idx]


def _segment_table_async(points, labels, flow_pd, flow_gt, z_min, out, max_segments):
    """icpflow_seq_segment_table of one cloud, enqueued on the current stream: `out` (float64 device tensor of
    max_segments * 16 + 1 words) receives the table and, in the low half of its last word, the int32 segment count."""
    import ctypes
    from . import utils_eval
    _lib.require_gpu(points, labels, flow_pd, flow_gt)
    if (flow_pd is None) != (flow_gt is None):
        raise ValueError("segment_table: flow_pd and flow_gt are given together or not at all")
    dev = points.device
    zmin = float("-inf") if z_min is None else utils_eval._threshold_for(z_min, points)
    pts = points[:, 0:3].to(torch.float64).contiguous()
    n = pts.shape[0]
    lab = labels.to(dev).contiguous().float()
    if lab.shape != (n,):
        raise ValueError(f"segment_table: {tuple(lab.shape)} labels for {n} points")
    gt = pd = None
    if flow_gt is not None:
        gt = flow_gt[:, 0:3].to(device=dev, dtype=torch.float64).contiguous()
        pd = flow_pd[:, 0:3].to(device=dev, dtype=torch.float32).contiguous()
        if gt.shape[0] != n or pd.shape[0] != n:
            raise ValueError(f"segment_table: {gt.shape[0]} / {pd.shape[0]} flow rows for {n} points")
    with torch.cuda.device(dev):
        need = int(_lib._L.icpflow_seq_segment_table_workspace_bytes(n, int(max_segments)))
        ws = _lib.workspace(dev, need)
        _lib.call("icpflow_seq_segment_table", _lib.ptr(pts), _lib.ptr(lab), n, _lib.ptr(gt), _lib.ptr(pd), zmin, _lib.ptr(out),
                  int(max_segments), ctypes.c_void_p(out.data_ptr() + int(max_segments) * _lib.SEG_COLS * 8), _lib.ptr(ws),
                  ctypes.c_size_t(ws.numel()), _lib.stream(dev))


def _count(word, max_segments):
    num = int(np.asarray(word).view(np.int32)[0])
    if num < 0:
        raise RuntimeError(f"segment_table: {-num} distinct labels, the table holds max_segments = {max_segments} (at most 4096)")
    return num


def segment_table(points, labels, flow_pd=None, flow_gt=None, z_min=None, max_segments=1024):
    """icpflow_seq_segment_table (csrc/segeval.hip) on GPU tensors: per distinct label, ascending, the 16 columns of
    include/icpflow_hip.h -- label, rows, kept rows (z > z_min), sum of the end point error, the four predicate counts, the
    coordinate sums and the sums of x + flow.  Without flows: label, rows, kept rows and the coordinate sums only.
    -> (float64 device tensor [S,16], S).  There is no CPU path."""
    _lib.require_gpu(points, labels, flow_pd, flow_gt)
    out = torch.empty(int(max_segments) * _lib.SEG_COLS + 1, dtype=torch.float64, device=points.device)
    _segment_table_async(points, labels, flow_pd, flow_gt, z_min, out, max_segments)
    num = _count(out[-1:].cpu().numpy(), max_segments)
    return out[: num * _lib.SEG_COLS].view(num, _lib.SEG_COLS), num


def euler_zyx_deg(R):
    """scipy's Rotation.from_matrix(R).as_euler("zyx", degrees=True) (utils_flow.py:124) in closed form, for a rotation matrix:
    extrinsic turns about z, y, x, R = Rx(c) Ry(b) Rz(a) -> [a, b, c] with b in [-90, 90].  (scipy first replaces a matrix
    that is not orthogonal by the nearest rotation; this does not.)"""
    R = np.asarray(R, dtype=np.float64)
    b = np.arctan2(R[0, 2], np.hypot(R[0, 0], R[0, 1]))
    a = np.arctan2(-R[0, 1], R[0, 0])
    c = np.arctan2(-R[1, 2], R[2, 2])
    return np.degrees(np.array([a, b, c]))


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else (None if a is None else np.asarray(a))


def segment_report(src_table, dst_table, pairs=None, transformations=None):
    """The host half of flow_evaluation: the two tables (numpy [S,16], [D,16]) -> SegmentReport.  The fractions are float32
    means of 0/1 flags (count / n rounded once), the mean error Σe / n in float64; a segment without a kept row gets NaN."""
    t, d = np.asarray(src_table, np.float64).reshape(-1, 16), np.asarray(dst_table, np.float64).reshape(-1, 16)
    S = len(t)
    n = t[:, 2].astype(np.int64)
    with np.errstate(all="ignore"):
        nf = n.astype(np.float64)
        epe = t[:, 3] / nf
        frac = [(t[:, 4 + k].astype(np.float32) / n.astype(np.float32)).astype(np.float32) for k in range(4)]
        mean_i = t[:, 8:11] / nf[:, None]
        moved = t[:, 11:14] / nf[:, None]
        translation = np.sqrt(((moved - mean_i) ** 2).sum(axis=1))
        where = {float(lab): k for k, lab in enumerate(d[:, 0])}
        at = np.array([where.get(float(lab), -1) for lab in t[:, 0]], dtype=np.int64)
        len_j = np.where(at >= 0, d[np.maximum(at, 0), 1] if len(d) else 0.0, 0.0).astype(np.int64) if S else np.zeros(0, np.int64)
        mean_j = np.full((S, 3), np.nan)
        if len(d):
            has = at >= 0
            mean_j[has] = d[at[has], 8:11] / d[at[has], 2][:, None]
    pair_index = np.full(S, -1, np.int64)
    matched = np.full(S, -1.0)
    rot = np.full((S, 3), np.nan)
    if pairs is not None and len(pairs):
        pairs = np.asarray(pairs)
        for k, lab in enumerate(t[:, 0]):
            idx = np.flatnonzero(pairs[:, 0] == lab)        # utils_flow.py:107-109
            if len(idx) == 1:
                pair_index[k], matched[k] = idx[0], pairs[idx[0], 1]
                if transformations is not None:
                    rot[k] = euler_zyx_deg(np.asarray(transformations)[idx[0]][0:3, 0:3])
    return SegmentReport(label=t[:, 0].copy(), rows=t[:, 1].astype(np.int64), n=n, sum_e=t[:, 3].copy(), epe=epe, accs=frac[0], accr=frac[1], outlier=frac[2],
                         routlier=frac[3], len_j=len_j, mean_i=mean_i, mean_j=mean_j, pair_index=pair_index, matched_dst=matched,
                         translation=translation, rotation_zyx_deg=rot, moved=moved)


def segment_lines(report, moved, pose=None, transformations=None, pairs=None):
    """The text the reference's flow_evaluation prints (utils_flow.py:97-124): the `eval segment:` line of every matched
    segment with label >= 0, and the block of a segment whose EPE exceeds 2.0.  Segments without a kept row do not exist for
    the reference (debug_frame crops the labels before np.unique) and print nothing."""
    lines = []
    for k in range(len(report)):
        unq, m = int(report.label[k]), int(report.n[k])
        if unq < 0 or m == 0:
            continue
        idx = int(report.pair_index[k])
        if idx >= 0:
            lines.append(f"eval segment: {unq:3d}, epe: {report.epe[k]:.4f}, i: {int(pairs[idx, 0]):3d}, j: {int(pairs[idx, 1]):3d}; "
                         f"len_i: {m:6d}, len_j: {int(report.len_j[k]):6d}, mean_i: {report.mean_i[k]}, mean_j: {report.mean_j[k]}")
        if report.epe[k] > LARGE_EPE:
            text = lambda *a: lines.append(" ".join(str(v) for v in a))    # noqa: E731  (what print() writes)
            text("predictions with substantially large flow errors")
            text("matched pair: ", unq, pairs[idx] if idx >= 0 else np.zeros((0, 10)), {m}, {int(report.len_j[k])})
            text("pose: ", pose)
            text("transform: ", transformations[idx] if idx >= 0 else np.zeros((0, 4, 4)))
            text("translation: ", moved[k], report.mean_i[k], report.translation[k])
            text("rotation: ", report.rotation_zyx_deg[k] if idx >= 0 else np.zeros((0, 3)))
    return lines


def flow_evaluation(src_points, dst_points, src_labels, dst_labels, flow_pd, flow_gt, pose, transformations, pairs=None,
                    z_min=None, verbose=False, max_segments=1024):
    """The reference's per-segment evaluation (utils_flow.py:72-150; its name and argument order) on GPU tensors: two calls
    of icpflow_seq_segment_table -- the source cloud with the flows, cropped at z > z_min like utils_debug.py:37-46, and the
    destination cloud without -- and ONE read-back of the two tables.  The labels of the two clouds come from a joint
    clustering, so a source segment's len_j and mean_j are those of the destination rows with the same label
    (utils_flow.py:88-91).  -> SegmentReport; verbose=True prints the reference's lines.  Nothing is visualised."""
    _lib.require_gpu(src_points, dst_points, src_labels, dst_labels, flow_pd, flow_gt)
    dev = src_points.device
    words = int(max_segments) * _lib.SEG_COLS + 1
    out = torch.empty(2 * words, dtype=torch.float64, device=dev)
    _segment_table_async(src_points, src_labels, flow_pd, flow_gt, z_min, out[:words], max_segments)
    _segment_table_async(dst_points, dst_labels, None, None, None, out[words:], max_segments)
    host = out.cpu().numpy()              # the one read-back of the tables
    S, D = _count(host[words - 1: words], max_segments), _count(host[2 * words - 1:], max_segments)
    pairs, transformations, pose = _host(pairs), _host(transformations), _host(pose)
    report = segment_report(host[: S * 16], host[words: words + D * 16], pairs, transformations)
    report.lines = segment_lines(report, report.moved, pose, transformations, pairs)
    if verbose:
        for line in report.lines:
            print(line)
    return report

"""Object pseudo labels: an oriented box per cluster and a box, a velocity and a heading per matched pair of a registered frame
pair (include/icpflow_hip.h, "8(j) object boxes"; csrc/boxes.hip).  No counterpart in the reference.

The box of a cluster is the bounding rectangle, among A directions of [0, 90) degrees, with the most points within `delta`
of one of its sides -- the rule that follows the two visible faces of a vehicle, where a minimum-area rule follows the
hypotenuse of the L as often as its legs.  `delta` defaults to utils_eval.RESIDUAL_EDGES[1], 0.1 m; like KEEP of
the trust byte it is a stated policy, not a metric of the reference.

Everything stays on the device until `Objects` reads the table back, once.  There is no CPU path."""
import ctypes
import math

import numpy as np

BOX_DELTA = 0.1               # utils_eval.RESIDUAL_EDGES[1]
BOX_DIRECTIONS = 90
SWEEP_SECONDS = 0.1
MIN_SPEED = 0.5               # m/s: what separates static from dynamic in the three-way EPE


def box_directions(A=BOX_DIRECTIONS):
    """float32 [A, 2]: (cos, sin) of k (pi / 2) / A, taken in float64 and narrowed -- the table icpflow_segment_boxes is given"""
    a = np.arange(int(A), dtype=np.float64) * (math.pi / 2) / int(A)
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def cluster_table_device(points, labels, Lmax=4096):
    """icpflow_cluster_table enqueued on the current stream, nothing read back -> (points float32 [n, 3], order int64 [n],
    table float64 [Lmax, 9], num int32 [1]): what segment_boxes_device takes as `table`"""
    import torch
    from . import _lib
    _lib.require_gpu(points, labels)
    if points.dim() != 2 or points.shape[1] < 3:
        raise ValueError(f"cluster_table: points {tuple(points.shape)}, expected [n, >= 3]")
    p = points[:, 0:3].to(torch.float32).contiguous()
    lab = labels.to(torch.float32).contiguous()
    n, device, Lmax = int(p.shape[0]), p.device, int(Lmax)
    if lab.shape != (n,) or lab.device != device:
        raise ValueError(f"cluster_table: labels {tuple(lab.shape)} on {lab.device} for {n} rows on {device}")
    order = torch.empty(n, dtype=torch.int64, device=device)
    table = torch.empty((Lmax, 9), dtype=torch.float64, device=device)
    num = torch.empty(1, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        ws = _lib.workspace(device, int(_lib._L.icpflow_cluster_table_workspace_bytes(n, Lmax)))
        _lib.call("icpflow_cluster_table", _lib.ptr(p), _lib.ptr(lab), n, _lib.ptr(order), _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(ws),
                  ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return p, order, table, num


def segment_boxes_device(points, labels, delta=BOX_DELTA, A=BOX_DIRECTIONS, Lmax=4096, table=None, dirs=None):
    """icpflow_segment_boxes enqueued on the current stream, nothing read back.  points [n, >= 3], labels [n]: device tensors;
    table: what cluster_table_device returned for them (None: it is run here); dirs: float32 [A, 2] of the caller's (None:
    box_directions(A)).  -> (boxes float64 [Lmax, 16], num int32 [1]) on the device; rows of `boxes` from num on are not
    written."""
    import torch
    from . import _lib
    _lib.require_gpu(points, labels)
    p, order, ctable, num = cluster_table_device(points, labels, Lmax) if table is None else table
    n, device, Lmax = int(p.shape[0]), p.device, int(ctable.shape[0])
    d = np.ascontiguousarray(box_directions(A) if dirs is None else dirs, dtype=np.float32).reshape(-1, 2)
    boxes = torch.empty((Lmax, _lib.BOX_COLS), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_segment_boxes_workspace_bytes(n, Lmax, len(d)))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_segment_boxes", _lib.ptr(p), n, _lib.ptr(order), _lib.ptr(ctable), _lib.ptr(num), Lmax, d.ctypes.data_as(ctypes.c_void_p),
                  len(d), float(delta), _lib.ptr(boxes), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return boxes, num


def pair_objects_device(boxes_src, num_src, pairs, transformations, boxes_dst=None, num_dst=None, seconds=SWEEP_SECONDS, min_speed=MIN_SPEED):
    """icpflow_pair_objects enqueued on the current stream, nothing read back.  boxes_src, num_src (and boxes_dst, num_dst, or
    both None): what segment_boxes_device returned for the two clouds; pairs [P, >= 2] (columns 0 and 1 the labels of a matched
    pair) and transformations [P, 4, 4] as the registration leaves them.  -> (objects float64 [P, 24], counts int64 [4]) on
    the device."""
    import torch
    from . import _lib
    _lib.require_gpu(boxes_src, num_src, pairs, transformations, boxes_dst, num_dst)
    device, Lmax = boxes_src.device, int(boxes_src.shape[0])
    for name, b in (("boxes_src", boxes_src), ("boxes_dst", boxes_dst)):
        if b is not None and (b.dtype != torch.float64 or tuple(b.shape) != (Lmax, _lib.BOX_COLS) or not b.is_contiguous()):
            raise ValueError(f"pair_objects: {name} {tuple(b.shape)} {b.dtype}, expected contiguous float64 [{Lmax}, {_lib.BOX_COLS}]")
    if (boxes_dst is None) != (num_dst is None):
        raise ValueError("pair_objects: the destination's boxes and their number come together or not at all")
    P = int(pairs.shape[0])
    rows = T = None
    stride = 2
    if P > 0:
        if pairs.dim() != 2 or pairs.shape[1] < 2 or tuple(transformations.shape) != (P, 4, 4):
            raise ValueError(f"pair_objects: pairs {tuple(pairs.shape)}, transformations {tuple(transformations.shape)}, expected [P, >= 2] and [P, 4, 4]")
        rows, T = pairs.to(torch.float32).contiguous(), transformations.to(torch.float32).contiguous()
        stride = int(rows.shape[1])
    if any(x is not None and x.device != device for x in (num_src, boxes_dst, num_dst, rows, T)):
        raise ValueError("pair_objects: every tensor on the same device")
    params = _lib.ObjectParams.defaults(seconds=seconds, min_speed=min_speed)
    objects = torch.empty((P, _lib.OBJECT_COLS), dtype=torch.float64, device=device)
    counts = torch.empty(_lib.OBJECT_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.call("icpflow_pair_objects", _lib.ptr(boxes_src), _lib.ptr(num_src), _lib.ptr(boxes_dst), _lib.ptr(num_dst), Lmax, _lib.ptr(rows), P,
                  stride, _lib.ptr(T), ctypes.byref(params), _lib.ptr(objects) if P else None, _lib.ptr(counts), _lib.stream(device))
    return objects, counts


COUNT_NAMES = ("objects", "movers", "pairs_without_source_segment", "pairs_without_destination_segment")


class Objects:
    """The object rows of one frame pair on the host (icpflow_pair_objects' table and counts, read back once)."""

    def __init__(self, rows, counts, seconds=SWEEP_SECONDS, min_speed=MIN_SPEED):
        self.rows = np.asarray(rows, np.float64).reshape(-1, 24)
        self.counts = np.asarray(counts, np.int64).reshape(4)
        self.seconds, self.min_speed = float(seconds), float(min_speed)

    @classmethod
    def read(cls, objects, counts, seconds=SWEEP_SECONDS, min_speed=MIN_SPEED):
        """the two device tensors of pair_objects_device in ONE transfer (the counts are exact in a float64)"""
        import torch
        host = torch.cat([objects.reshape(-1), counts.to(torch.float64)]).cpu().numpy()
        return cls(host[:-4], np.rint(host[-4:]), seconds, min_speed)

    def summary(self):
        return dict({k: int(v) for k, v in zip(COUNT_NAMES, self.counts)}, pairs=len(self.rows))

    def largest_centre_gap(self):
        """metres; None when no object has a destination box"""
        gap = self.rows[:, 21][(self.rows[:, 3] >= 0) & (self.rows[:, 21] >= 0) & (self.rows[:, 22] > 0)]
        return float(np.sqrt(gap.max())) if len(gap) else None

    def as_list(self):
        """one dict per pair with a source box, in the order of the pairs"""
        out = []
        for p, r in enumerate(self.rows):
            if r[22] <= 0:
                continue
            out.append(dict(pair=p, label_src=float(r[0]), label_dst=float(r[1]), centre=[float(v) for v in r[4:7]],
                            size=[float(v) for v in r[16:19]], yaw=math.atan2(r[20], r[19]), velocity=[float(v) for v in r[10:13]],
                            speed=math.sqrt(r[13]), moving=bool(r[14]), centre_gap=math.sqrt(r[21]) if r[21] >= 0 else None,
                            points_src=int(r[22]), points_dst=int(r[23])))
        return out


def format_objects(objects):
    """`Objects.as_list()` as lines of text"""
    lines = ["  label_src  label_dst        x        y        z   length    width   height   yaw_deg    speed  moving  centre_gap  points"]
    for e in objects:
        gap = "         -" if e["centre_gap"] is None else f"{e['centre_gap']:10.3f}"
        lines.append(f"{e['label_src']:11g}{e['label_dst']:11g}{e['centre'][0]:9.2f}{e['centre'][1]:9.2f}{e['centre'][2]:9.2f}"
                     f"{e['size'][0]:9.2f}{e['size'][1]:9.2f}{e['size'][2]:9.2f}{math.degrees(e['yaw']):10.1f}{e['speed']:9.2f}"
                     f"{'yes' if e['moving'] else 'no':>8}  {gap}{e['points_src']:8d}")
    return lines

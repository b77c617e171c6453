"""Scene-flow accuracy metrics of the reference's evaluation (utils_eval.py:65-182), numpy on the
host like the reference's.  Pinned by tests/golden/g9_epe.npz.

The evaluation of a whole sequence -- crop_data / calculate_metrics, utils_eval.py:24-63 and 185-368 -- runs on the GPU
(icpflow_seq_metrics, csrc/seqeval.hip): one pass over the points, one table of F x 6 x 6 numbers back, from which the
reference's meters are updated row by row.  Pinned by tests/golden/g13_seqeval_*.npz.

Per class, per speed bucket and per error split -- the Argoverse 2 way of reporting, for which the reference carries the
tables (dataset_argo.py:145-217) and uses six names of them: `class_table` (icpflow_seq_class_table, csrc/classeval.hip), one
more pass over the rows and one small table back; `ClassTable` adds, groups and prints it, `ClassTable.threeway` is the
three-way EPE.  The names and groups below are pinned by tests/golden/g16_argo_classes.json.

The bucket-normalised EPE Argoverse 2 has been ranked by since its 2024 challenge (Khatri et al., ECCV 2024): `bucket_table`
(icpflow_seq_bucket_table, csrc/bucketeval.hip) is one more pass and one table of 33 rows x 51 speed buckets back; `BucketTable`
adds and groups it, `bucketed_epe` is the metric per challenge class.  A restatement of the published method, unpinned
against the `bucketed_scene_flow_eval` package (COVERAGE.md, named deviations).

Without ground truth: `nn_residual` (icpflow_nn_residual, csrc/nnresid.hip) is the truncated nearest-neighbour residual of a
warped cloud against the next one -- a hashed grid over the whole frame and an exact radius-bounded search on the GPU;
`ResidualTable` adds and prints it, `chamfer` is the two directions.  A label-free proxy, not a metric of the reference
(COVERAGE.md, named deviations).  `segment_residual` (icpflow_nn_residual_segments, csrc/segresid.hip) is the same residual per
segment of the source, before and after the flow, against one grid: `SegmentResidual.worst` names the clusters that fit badly;
`sight_image` / `line_of_sight` / `segment_sight` (icpflow_sight_*, csrc/sight.hip) ask the destination sweep whether such a
cluster was put where the sweep saw free space or merely went out of view: `SegmentSight.annotate` adds the verdict.
`flow_trust` (icpflow_flow_trust, csrc/trust.hip) spreads both verdicts over the rows: one byte per source point from the two
tables and the per-row arrays, `trust_keep` its KEEP bit -- a stated policy for flows saved as pseudo labels, not a metric."""
import numpy as np

METRIC_NAMES = ("epe", "accs", "accr", "outlier", "Routlier")


def compute_epe_test(flow_pred, flow_gt, mask=None):
    """utils_eval.py:137-182 -> (EPE3D, strict accuracy, relaxed accuracy, outliers, R-outliers).

    Per point e = |gt - pred|, r = e / (|gt| + 1e-20):  strict e < 0.05 or r < 0.05;  relaxed
    e < 0.1 or r < 0.1;  outlier e > 0.3 or r > 0.1;  R-outlier e > 0.3 and r > 0.3.  Fractions are
    float32 means, as in the reference."""
    flow_pred, flow_gt = np.asarray(flow_pred), np.asarray(flow_gt)
    assert flow_gt.shape[-1] == 3 and flow_pred.shape[-1] == 3
    if mask is not None:
        keep = np.asarray(mask) > 0
        flow_gt, flow_pred = flow_gt[keep], flow_pred[keep]
    err = np.linalg.norm(flow_gt - flow_pred, axis=-1)
    rel = err / (np.linalg.norm(flow_gt, axis=-1) + 1e-20)

    def frac(cond):
        return cond.astype(np.float32).mean()

    return (err.mean(), frac((err < 0.05) | (rel < 0.05)), frac((err < 0.1) | (rel < 0.1)),
            frac((err > 0.3) | (rel > 0.1)), frac((err > 0.3) & (rel > 0.3)))


def average_meter(errors, nums):
    """utils_eval.py:65-80: point-count weighted mean of per-frame errors."""
    assert len(errors) == len(nums)
    return sum(e * n for e, n in zip(errors, nums)) / sum(nums)


class AverageMeter:
    """utils_eval.py:82-135: running point-weighted averages of the five metrics; keeps the
    per-frame values (`*_data`) like the reference."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.num = 0
        self.num_data = []
        for m in METRIC_NAMES:
            setattr(self, m + "_sum", 0.0)
            setattr(self, m + "_avg", 0.0)
            setattr(self, m + "_data", [])

    def update(self, epe, accs, accr, outlier, Routlier, num):
        self.num += num
        self.num_data.append(num)
        for m, v in zip(METRIC_NAMES, (epe, accs, accr, outlier, Routlier)):
            total = getattr(self, m + "_sum") + v * num
            setattr(self, m + "_sum", total)
            setattr(self, m + "_avg", total / self.num)
            getattr(self, m + "_data").append(v)

    def averages(self):
        return {m: float(getattr(self, m + "_avg")) for m in METRIC_NAMES}


METRIC_CLASSES = ("overall", "static", "static_bg", "static_fg", "dynamic", "dynamic_fg")


def metric_table_names(num_frames):
    """The keys of the reference's table in the order main.py:173-180 creates them: per class, row 0 (per point over all
    gaps), rows 1 .. num_frames - 1 (per gap), row num_frames (per scene)."""
    return [f"{metric}_{k:d}" for metric in METRIC_CLASSES for k in range(0, num_frames + 1)]


def new_metric_table(num_frames):
    """main.py:173-180: a fresh AverageMeter under every name."""
    return {name: AverageMeter() for name in metric_table_names(num_frames)}


def format_metric_table(metrics_per_frame, num_frames):
    """The reference's closing lines (main.py:288-296) as one string; the run of blanks inside a line is the
    continuation of the reference's source line, which is part of its string."""
    gap = ", " + " " * 18
    lines = ["################# Results over the entire dataset #####################################"]
    for k in range(0, num_frames + 1):
        for metric in METRIC_CLASSES:
            name = metric + f"_{k:d}"
            m = metrics_per_frame[name]
            lines.append(f"{name:12}, EPE3D: {m.epe_avg:.6f}{gap}ACC3DS: {m.accs_avg:.6f}{gap}ACC3DR: {m.accr_avg:.6f}{gap}"
                         f"Outlier: {m.outlier_avg:.6f}{gap}Routlier: {m.Routlier_avg:.6f}.")
    return "\n".join(lines)


def _crop_mask(args, raw_points):
    """utils_eval.py:33-38 with the array's own comparison (numpy rounds the threshold to a float32 array's type,
    torch does the same)."""
    import torch
    absf = torch.abs if isinstance(raw_points, torch.Tensor) else np.abs
    keep = (absf(raw_points[:, 0]) < args.range_x) & (absf(raw_points[:, 1]) < args.range_y)
    if not args.eval_ground:
        keep = keep & (raw_points[:, 2] > args.range_z + args.ground_slack)
    return keep


def crop_data(args, data, pred):
    """utils_eval.py:24-63: crop the scene in x and y and, unless args.eval_ground, drop what lies below
    range_z + ground_slack.  numpy arrays or device tensors (a gather per array on whichever side they live;
    calculate_metrics does not call this -- its kernel applies the same test row by row)."""
    keep = _crop_mask(args, data["raw_points"])
    out = dict(data)
    for k in ("raw_points", "time_indice", "sd_labels", "fb_labels", "scene_flow"):
        out[k] = data[k][keep]
    return out, pred[keep]


def _threshold_for(value, raw_points):
    """A crop threshold as numpy compares it with the sample's coordinates: a float32 (float16) array is compared with the
    threshold rounded to its type; the kernel compares the exactly widened coordinate with this number in fp64."""
    import torch
    dt = raw_points.dtype
    if isinstance(raw_points, torch.Tensor):
        dt = {torch.float32: np.float32, torch.float16: np.float16}.get(dt, np.float64)
    dt = np.dtype(dt)
    if dt.kind == "f" and dt.itemsize < 8:
        return float(np.asarray(value, dtype=np.float64).astype(dt))
    return float(value)


def _binary_labels(labels, device):
    """Labels as the kernel reads them: 0, 1, or 2 for anything that equals neither (`== 0` / `== 1` on the sample's own type)."""
    import torch
    from . import utils_loading
    if isinstance(labels, torch.Tensor):
        t = labels.to(device)
        return torch.where(t == 0, 0, torch.where(t == 1, 1, 2)).to(torch.int32).contiguous()
    a = np.asarray(labels)
    return utils_loading.to_device(np.where(a == 0, 0, np.where(a == 1, 1, 2)).astype(np.int32), torch.int32, device)


def narrow_time_indices(time_indice, F):
    """Time indices as the kernels read them (int32), narrowed the way _binary_labels narrows the labels: compared on the sample's
    own type first.  A value that equals an integer of [0, F) -- the reference's `time_indice == j` is true for one j -- keeps
    it; every other value (an int64 beyond int32 that a plain cast would wrap into [0, F), a fraction that it would truncate, NaN,
    +-inf) becomes -1, which the kernels count as OUTSIDE and in no cell.  numpy array or tensor -> the same kind, int32."""
    import torch
    F = int(F)
    if isinstance(time_indice, torch.Tensor):
        t = time_indice if time_indice.is_floating_point() else time_indice.to(torch.int64)
        inside = (t >= 0) & (t < F)
        if t.is_floating_point():
            inside = inside & (t == torch.floor(t))
        return torch.where(inside, t, torch.full_like(t, -1)).to(torch.int32)
    a = np.asarray(time_indice)
    if a.dtype == object:
        raise TypeError("an object array cannot be evaluated on the device")
    if a.dtype.kind != "f":
        a = a.astype(np.int64)
    with np.errstate(invalid="ignore"):
        inside = (a >= 0) & (a < F)
        if a.dtype.kind == "f":
            inside = inside & (a == np.floor(a))
        return np.where(inside, a, -1).astype(np.int32)


def _time_indices(time_indice, F, device):
    """narrow_time_indices on the device the call runs on"""
    import torch
    from . import utils_loading
    if isinstance(time_indice, torch.Tensor):
        return narrow_time_indices(utils_loading.to_device(time_indice, time_indice.dtype, device), F).contiguous()
    return utils_loading.to_device(narrow_time_indices(time_indice, F), torch.int32, device)


def _crop_arguments(args, raw):
    """calculate_metrics' crop as the kernels take it -> (ICPFLOW_SEQ_CROP_*, range_x, range_y, z_min)"""
    from . import _lib
    if args.eval_ground:                 # utils_eval.py:186-189: no crop at all
        return _lib.SEQ_CROP_NONE, 0.0, 0.0, 0.0
    return (_lib.SEQ_CROP_XYZ, _threshold_for(args.range_x, raw), _threshold_for(args.range_y, raw),
            _threshold_for(args.range_z + args.ground_slack, raw))


def sequence_table(args, data, flow_seq):
    """icpflow_seq_metrics on one sequence -> (table int64 [F,6,6] numpy, sum of e float64 [F,6] numpy, kept points of
    frame 0, rows with a time index outside [0,F)).  Inputs may live on either side; with device tensors the only
    device -> host copy is the table (F * 36 + 2 words, one copy).
    OUTSIDE is every time index that equals no integer of [0, F) on the sample's own type -- the reference's `time_indice == j`
    holds for no j: -1, F, an int64 such as 2^32 + 1 (never wrapped to 1), 1.5 (never truncated to 1), NaN.  Such a row is
    counted there, in no cell and not in kept0 (narrow_time_indices); class_table and bucket_table read it the same way."""
    import ctypes
    import torch
    from . import _lib, utils_loading
    device = utils_loading._device_for(flow_seq, data["raw_points"], data["scene_flow"])
    F = int(args.num_frames)
    raw = data["raw_points"]
    pts = utils_loading.to_device(raw, torch.float64, device)[:, 0:3].contiguous()
    m = pts.shape[0]
    tim = _time_indices(data["time_indice"], F, device)
    sd, fb = _binary_labels(data["sd_labels"], device), _binary_labels(data["fb_labels"], device)
    gt = utils_loading.to_device(data["scene_flow"], torch.float64, device)[:, 0:3].contiguous()
    pred = utils_loading.to_device(flow_seq, torch.float32, device)[:, 0:3].contiguous()
    for name, t in (("time_indice", tim), ("sd_labels", sd), ("fb_labels", fb), ("scene_flow", gt), ("flow_seq", pred)):
        if t.shape[0] != m:
            raise ValueError(f"{name}: {t.shape[0]} rows for {m} points")
    crop, rx, ry, zmin = _crop_arguments(args, raw)
    out = torch.empty(F * 36 + 2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_seq_metrics_workspace_bytes(m, F))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_seq_metrics", _lib.ptr(pts), _lib.ptr(tim), _lib.ptr(sd), _lib.ptr(fb), _lib.ptr(gt), _lib.ptr(pred), m, F,
                  crop, rx, ry, zmin, _lib.ptr(out), ctypes.c_void_p(out.data_ptr() + F * 36 * 8), _lib.ptr(ws),
                  ctypes.c_size_t(ws.numel()), _lib.stream(device))
    host = out.cpu().numpy()             # the one read-back
    table = host[: F * 36].reshape(F, 6, 6)
    esum = np.ascontiguousarray(table[:, :, 1]).view(np.float64)
    return table, esum, int(host[F * 36]), int(host[F * 36 + 1])


def _cell_metrics(table, esum, j, c):
    """The five numbers compute_epe_test returns for one cell, in the reference's types: the mean error float64, the four
    fractions float32 means of 0/1 flags (count / n rounded once: exact sums below 2^24 points).  An empty cell gives what numpy's
    mean of nothing gives, NaN."""
    n = int(table[j, c, 0])
    if n == 0:
        return (np.float64("nan"),) + (np.float32("nan"),) * 4
    return (np.float64(esum[j, c]) / n,) + tuple(np.float32(np.float32(int(table[j, c, 2 + k])) / np.float32(n)) for k in range(4))


def calculate_metrics(args, data, flow_seq, metrics_per_frame):
    """utils_eval.py:185-368 with the reference's signature and its meter updates, row by row: `data` is the sample
    (raw_points, time_indice, sd_labels, fb_labels, scene_flow), `flow_seq` the predicted flow of every point (zeros for
    frame 0), `metrics_per_frame` the dict of AverageMeters under metric_table_names(args.num_frames); args carries
    num_frames, eval_ground, range_x, range_y, range_z, ground_slack.  The per-point work is icpflow_seq_metrics (GPU; numpy
    arrays are uploaded, device tensors are used where they are and only the table comes back); there is no CPU path.

    The reference's quirks, kept:
      * `overall_0` is weighted with the number of cropped points INCLUDING frame 0 (utils_eval.py:275, len(flow_seq)),
        although its values average the points of the other frames only;
      * `overall_j` and `static_j` (and `static_0`, `static_F`) are updated even when the class is empty -- with NaN and weight 0, after
        which that meter's sums stay NaN; the other four classes skip an empty row (utils_eval.py:226, 234, 242, 254);
      * the per-scene rows (`*_F`) are weighted 1 per sequence, whatever its size;
      * with eval_ground nothing is cropped, not even in x and y (utils_eval.py:186-189);
      * the weights keep the reference's types (len() is an int, sum(mask) a numpy integer): numpy's promotion of a float32 fraction
        times the weight follows from them.
    Not kept: the reference prints three lines per gap; pass args.if_verbose to get them."""
    table, esum, kept0 = checked_sequence_table(args, data, flow_seq)
    return update_meters(args, metrics_per_frame, table, esum, kept0)


def checked_sequence_table(args, data, flow_seq):
    """The device half of calculate_metrics with its refusals: sequence_table, no time index outside [0, F), every frame
    present after the crop (utils_eval.py:197-198).  -> (table, esum, kept0) for update_meters"""
    F = int(args.num_frames)
    table, esum, kept0, outside = sequence_table(args, data, flow_seq)
    if outside:
        raise ValueError(f"{outside} points have a time index outside [0, {F})")
    present = int(kept0 > 0) + sum(int(table[j, 0, 0] > 0) for j in range(1, F))
    assert present == args.num_frames, f"{present} frames have points after the crop, args.num_frames is {args.num_frames}"   # utils_eval.py:197-198
    return table, esum, kept0


def update_meters(args, metrics_per_frame, table, esum, kept0):
    """The host half of calculate_metrics: one sequence's table (icpflow_seq_metrics: counts int64 [F,6,6], sums of e
    float64 [F,6], kept points of frame 0) -> the reference's meter updates (utils_eval.py:200-366)."""
    with np.errstate(all="ignore"):                      # (NaN rows of empty classes: the reference silences every warning)
        return _update_meters(args, metrics_per_frame, table, esum, kept0)


def _update_meters(args, metrics_per_frame, table, esum, kept0):
    F = int(args.num_frames)
    weight = lambda n: np.int64(n) if n else 0          # noqa: E731  (sum(mask): a numpy integer, the int 0 for an empty mask)
    for j in range(1, F):
        for c, metric in enumerate(METRIC_CLASSES):
            n = int(table[j, c, 0])
            if c >= 2 and n == 0:
                continue
            vals = _cell_metrics(table, esum, j, c)
            if getattr(args, "if_verbose", False) and c in (0, 1, 4):
                print(f"frame: {j:02d}, {metric:>7}, EPE3D: {vals[0]:.4f}, ACC3DS: {vals[1]:.4f}, ACC3DR: {vals[2]:.4f}, "
                      f"Outlier: {vals[3]:.4f}, Routlier: {vals[4]:.4f}")
            metrics_per_frame[f"{metric}_{j:d}"].update(*vals, n if c == 0 else weight(n))
    total = kept0 + int(table[0, 0, 0])                  # len(flow_seq) after the crop
    for row, per_scene in ((0, False), (F, True)):
        for c, metric in enumerate(METRIC_CLASSES):
            n = int(table[0, c, 0])
            if c >= 2 and n == 0:
                continue
            vals = _cell_metrics(table, esum, 0, c)
            w = 1 if per_scene else total if c == 0 else weight(n)
            metrics_per_frame[f"{metric}_{row:d}"].update(*vals, w)
    return metrics_per_frame


# ---- per class, per speed bucket, per error split ---------------------------------------------------------------------
# The public Argoverse 2 taxonomy in alphabetical order behind the name the reference's id table starts with (its id -1),
# by the POSITION the reference compares a file's pc1_classes with (dataset_argo.py:23-25, 69-70: position = id + 1, so a file
# value of 5 is BOLLARD to it).  A file value of -1 has no position: the row "UNLABELLED".
ARGO_CATEGORY_NAMES = (
    "BACKGROUND", "ANIMAL", "ARTICULATED_BUS", "BICYCLE", "BICYCLIST", "BOLLARD", "BOX_TRUCK", "BUS", "CONSTRUCTION_BARREL",
    "CONSTRUCTION_CONE", "DOG", "LARGE_VEHICLE", "MESSAGE_BOARD_TRAILER", "MOBILE_PEDESTRIAN_CROSSING_SIGN", "MOTORCYCLE",
    "MOTORCYCLIST", "OFFICIAL_SIGNALER", "PEDESTRIAN", "RAILED_VEHICLE", "REGULAR_VEHICLE", "SCHOOL_BUS", "SIGN", "STOP_SIGN",
    "STROLLER", "TRAFFIC_LIGHT_TRAILER", "TRUCK", "TRUCK_CAB", "VEHICULAR_TRAILER", "WHEELCHAIR", "WHEELED_DEVICE", "WHEELED_RIDER")
ARGO_CLASS_LO, ARGO_CLASS_ROWS = -1, 33             # rows: file values -1 .. 30, then everything else
ARGO_ROW_NAMES = ("UNLABELLED",) + ARGO_CATEGORY_NAMES + ("OTHER",)
# table rows (file value + 1) per meta category.  BACKGROUND is exactly what the reference's fb label makes background: file
# values -1, 5, 8, 9, 13, 21, 22.  File value 0 ("BACKGROUND" by position), ANIMAL, DOG and the last row are foreground in
# no named group.
ARGO_META_GROUPS = {"BACKGROUND": (0, 6, 9, 10, 14, 22, 23),
                    "PEDESTRIAN": (17, 18, 24, 29),
                    "SMALL_MOVERS": (4, 5, 15, 16, 30, 31),
                    "LARGE_MOVERS": (3, 7, 8, 12, 13, 19, 20, 21, 25, 26, 27, 28)}
ARGO_SPEED_EDGES = (0.5 * 0.1, 2.0 * 0.1)           # metres per frame at 10 Hz: 0.5 and 2 m/s
ARGO_ERROR_EDGES = (0.05, 0.1)                      # metres


class ClassTable:
    """icpflow_seq_class_table's numbers on the host: counts int64 [G,S,E] (class row, speed bucket, error split), esum and
    ssum float64 [G,S] (sums of e and of |gt|), kept0 (kept rows of frame 0), names (one per row, or None)."""

    def __init__(self, counts, esum, ssum, kept0=0, names=None):
        self.counts = np.array(counts, dtype=np.int64)
        self.esum, self.ssum = np.array(esum, dtype=np.float64), np.array(ssum, dtype=np.float64)
        self.kept0 = int(kept0)
        self.names = tuple(names) if names is not None else None
        G, S, _ = self.counts.shape
        assert self.esum.shape == (G, S) and self.ssum.shape == (G, S)

    @classmethod
    def zeros(cls, G, S, E):
        return cls(np.zeros((G, S, E), np.int64), np.zeros((G, S)), np.zeros((G, S)))

    @classmethod
    def from_words(cls, words, G, S, E, kept0=0):
        """the kernel's int64 [G][S][E + 2] -> ClassTable"""
        w = np.ascontiguousarray(np.asarray(words, dtype=np.int64).reshape(G, S, E + 2))
        return cls(w[:, :, :E], np.ascontiguousarray(w[:, :, E]).view(np.float64), np.ascontiguousarray(w[:, :, E + 1]).view(np.float64), kept0)

    def words(self):
        """-> int64 [G * S * (E + 2)], the kernel's layout (the sums as their bits)"""
        G, S, E = self.counts.shape
        w = np.empty((G, S, E + 2), np.int64)
        w[:, :, :E], w[:, :, E], w[:, :, E + 1] = self.counts, self.esum.view(np.int64), self.ssum.view(np.int64)
        return w.reshape(-1)

    def add(self, other):
        """Accumulate another sample's table: integers add exactly, the sums add in call order.  -> self"""
        if other.counts.shape != self.counts.shape:
            raise ValueError(f"class tables of {other.counts.shape} and {self.counts.shape} do not add")
        self.counts = self.counts + other.counts
        self.esum, self.ssum = self.esum + other.esum, self.ssum + other.ssum
        self.kept0 += other.kept0
        return self

    def _rows_sum(self, rows):
        """the rows added in ascending row order -> (counts [S,E], esum [S], ssum [S])"""
        _, S, E = self.counts.shape
        counts, esum, ssum = np.zeros((S, E), np.int64), np.zeros(S), np.zeros(S)
        for r in sorted(rows):
            counts, esum, ssum = counts + self.counts[r], esum + self.esum[r], ssum + self.ssum[r]
        return counts, esum, ssum

    def meta(self, groups):
        """Rows summed per named group ({name: rows}) in ascending row order; the rows in no group form OTHER, the last
        row.  -> ClassTable of len(groups) + 1 rows with `names`"""
        G = self.counts.shape[0]
        used = [r for rows in groups.values() for r in rows]
        if len(set(used)) != len(used) or any(not 0 <= r < G for r in used):
            raise ValueError("meta: every row belongs to at most one group and lies in the table")
        parts = [self._rows_sum(rows) for rows in groups.values()] + [self._rows_sum(set(range(G)) - set(used))]
        return ClassTable(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
                          self.kept0, tuple(groups) + ("OTHER",))

    def threeway(self, background=ARGO_META_GROUPS["BACKGROUND"]):
        """The three-way EPE over whatever was accumulated: FD = foreground rows (every row not in `background`) in a speed
        bucket >= 1, FS = foreground rows in bucket 0, BS = background rows in bucket 0; each (sum of e) / (rows), rows in
        ascending order, then buckets.  An empty component is NaN, and so is the mean then.  Dynamic background rows are in
        no component (the reference's six classes have none for them): their count is `n_BD`.
        -> dict(FD, FS, BS, mean, n_FD, n_FS, n_BS, n_BD)"""
        G = self.counts.shape[0]
        bg = sorted(set(background))
        fg = [r for r in range(G) if r not in set(bg)]
        n = self.counts.sum(axis=2)

        def part(rows, buckets):
            total, rows_n = 0.0, 0
            for r in rows:
                for s in buckets:
                    total, rows_n = total + self.esum[r, s], rows_n + int(n[r, s])
            return (total / rows_n if rows_n else float("nan")), rows_n

        moving = range(1, self.counts.shape[1])
        (fd, n_fd), (fs, n_fs), (bs, n_bs) = part(fg, moving), part(fg, (0,)), part(bg, (0,))
        return dict(FD=float(fd), FS=float(fs), BS=float(bs), mean=float((fd + fs + bs) / 3.0), n_FD=n_fd, n_FS=n_fs, n_BS=n_bs,
                    n_BD=int(n[bg][:, 1:].sum()))


def class_table(args, data, flow_seq, classes=None, speed_edges=ARGO_SPEED_EDGES, error_edges=ARGO_ERROR_EDGES, class_lo=ARGO_CLASS_LO,
                rows=ARGO_CLASS_ROWS):
    """icpflow_seq_class_table on one sample -> ClassTable of `rows` class rows (values class_lo .. class_lo + rows - 2 of
    `classes`, default data["classes"], one per point; everything else in the last row), len(speed_edges) + 1 speed buckets
    (|scene_flow| in metres per frame, lower edge inclusive) and len(error_edges) + 1 error splits, over the rows
    calculate_metrics counts: those that pass args' crop with a time index in [1, num_frames).  Inputs as for
    sequence_table; the one device -> host copy is the table.  There is no CPU path."""
    import ctypes
    import torch
    from . import _lib, utils_loading
    device = utils_loading._device_for(flow_seq, data["raw_points"], data["scene_flow"])
    F = int(args.num_frames)
    raw = data["raw_points"]
    pts = utils_loading.to_device(raw, torch.float64, device)[:, 0:3].contiguous()
    m = pts.shape[0]
    tim = _time_indices(data["time_indice"], F, device)
    cls = utils_loading.to_device(data["classes"] if classes is None else classes, torch.float64, device)
    gt = utils_loading.to_device(data["scene_flow"], torch.float64, device)[:, 0:3].contiguous()
    pred = utils_loading.to_device(flow_seq, torch.float32, device)[:, 0:3].contiguous()
    for name, t in (("time_indice", tim), ("classes", cls), ("scene_flow", gt), ("flow_seq", pred)):
        if t.shape[0] != m or (name == "classes" and t.dim() != 1):
            raise ValueError(f"{name}: {tuple(t.shape)} for {m} points")
    crop, rx, ry, zmin = _crop_arguments(args, raw)
    G = int(rows)
    speed, error = np.ascontiguousarray(speed_edges, dtype=np.float64).reshape(-1), np.ascontiguousarray(error_edges, dtype=np.float64).reshape(-1)
    S, E = len(speed) + 1, len(error) + 1
    edge_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if len(a) else None   # noqa: E731
    words = G * S * (E + 2)
    out = torch.empty(max(words, 0) + 2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_seq_class_table_workspace_bytes(m, G, S, E))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_seq_class_table", _lib.ptr(pts), _lib.ptr(tim), _lib.ptr(cls), _lib.ptr(gt), _lib.ptr(pred), m, F, crop, rx, ry,
                  zmin, float(class_lo), G, edge_ptr(speed), S, edge_ptr(error), E, _lib.ptr(out),
                  ctypes.c_void_p(out.data_ptr() + words * 8), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    host = out.cpu().numpy()             # the one read-back
    if int(host[words + 1]):
        raise ValueError(f"{int(host[words + 1])} points have a time index outside [0, {F})")
    return ClassTable.from_words(host[:words], G, S, E, kept0=int(host[words]))


def format_class_table(table, names=ARGO_ROW_NAMES, groups=ARGO_META_GROUPS, rate_hz=10.0, fine=False, speed_edges=ARGO_SPEED_EDGES,
                       error_edges=ARGO_ERROR_EDGES):
    """One line per non-empty (meta category, speed bucket): n, mean EPE, mean speed in m/s (|gt| per frame times rate_hz)
    and the shares of the error splits; with `fine`, the non-empty rows of the table itself follow.  The last line is the
    three-way EPE with the number of dynamic background rows, which are in none of its components."""
    def bounds(edges, scale, unit):
        e = [0.0] + [x * scale for x in edges] + [float("inf")]
        return [f"[{a:g}, {b:g}) {unit}" for a, b in zip(e, e[1:])]

    buckets = bounds(speed_edges, rate_hz, "m/s")
    splits = "/".join(f"e<{x:g}" for x in error_edges) + "/rest"

    def lines(t, row_names):
        out = []
        for g, name in enumerate(row_names):
            for s in range(t.counts.shape[1]):
                n = int(t.counts[g, s].sum())
                if n:
                    shares = " ".join(f"{c / n:.4f}" for c in t.counts[g, s])
                    out.append(f"{name:>32}, {buckets[s]:>16}, n: {n:8d}, EPE3D: {t.esum[g, s] / n:.6f}, speed: {t.ssum[g, s] / n * rate_hz:.4f} m/s, "
                               f"{splits}: {shares}")
        return out

    meta = table.meta(groups)
    text = ["################# Per class and speed bucket ##########################################"] + lines(meta, meta.names)
    if fine:
        text += ["################# Per category ########################################################"] + lines(table, names)
    tw = table.threeway(groups["BACKGROUND"]) if "BACKGROUND" in groups else table.threeway(())
    text.append(f"three-way EPE: {tw['mean']:.6f}, FD: {tw['FD']:.6f} (n {tw['n_FD']}), FS: {tw['FS']:.6f} (n {tw['n_FS']}), "
                f"BS: {tw['BS']:.6f} (n {tw['n_BS']}); dynamic background rows, in no component: {tw['n_BD']}")
    return "\n".join(text)


# ---- bucket-normalised EPE per class (Argoverse 2, 2024 challenge) ---------------------------------------------------------
# 51 speed buckets from 50 interior edges in metres per frame: 0.04, ..., 2.0 (0.4 ... 20 m/s at 10 Hz), lower edge
# inclusive; bucket 0 = [0, 0.04) is "static", bucket 50 = [2.0, inf).  The doubles numpy produces, handed over as they are.
ARGO_BUCKET_EDGES = tuple(float(x) for x in np.linspace(0.0, 2.0, 51)[1:])
# the challenge's five classes BY NAME (the publication's taxonomy); rows in no group -- ANIMAL, DOG, OTHER -- are reported
# as OTHER and enter neither mean
_ARGO_CHALLENGE_NAMES = {
    "BACKGROUND": ("UNLABELLED", "BACKGROUND", "BOLLARD", "CONSTRUCTION_BARREL", "CONSTRUCTION_CONE", "MOBILE_PEDESTRIAN_CROSSING_SIGN",
                   "SIGN", "STOP_SIGN"),
    "CAR": ("REGULAR_VEHICLE",),
    "OTHER_VEHICLES": ("ARTICULATED_BUS", "BOX_TRUCK", "BUS", "LARGE_VEHICLE", "MESSAGE_BOARD_TRAILER", "RAILED_VEHICLE", "SCHOOL_BUS",
                       "TRAFFIC_LIGHT_TRAILER", "TRUCK", "TRUCK_CAB", "VEHICULAR_TRAILER"),
    "PEDESTRIAN": ("OFFICIAL_SIGNALER", "PEDESTRIAN", "STROLLER", "WHEELCHAIR"),
    "WHEELED_VRU": ("BICYCLE", "BICYCLIST", "MOTORCYCLE", "MOTORCYCLIST", "WHEELED_DEVICE", "WHEELED_RIDER")}
assert all(n in ARGO_ROW_NAMES for names in _ARGO_CHALLENGE_NAMES.values() for n in names), "a challenge class names a row that does not exist"
ARGO_CHALLENGE_GROUPS = {group: tuple(sorted(ARGO_ROW_NAMES.index(n) for n in names)) for group, names in _ARGO_CHALLENGE_NAMES.items()}


class BucketTable:
    """icpflow_seq_bucket_table's numbers on the host: counts int64 [G,S] (class row, speed bucket), esum and ssum float64
    [G,S] (sums of e and of |gt|), kept0 (kept rows of frame 0), names (one per row, or None)."""

    def __init__(self, counts, esum, ssum, kept0=0, names=None):
        self.counts = np.array(counts, dtype=np.int64)
        self.esum, self.ssum = np.array(esum, dtype=np.float64), np.array(ssum, dtype=np.float64)
        self.kept0 = int(kept0)
        self.names = tuple(names) if names is not None else None
        assert self.counts.ndim == 2 and self.esum.shape == self.counts.shape and self.ssum.shape == self.counts.shape

    @classmethod
    def zeros(cls, G, S):
        return cls(np.zeros((G, S), np.int64), np.zeros((G, S)), np.zeros((G, S)))

    @classmethod
    def from_words(cls, words, G, S, kept0=0):
        """the kernel's int64 [G][S][3] -> BucketTable"""
        w = np.ascontiguousarray(np.asarray(words, dtype=np.int64).reshape(G, S, 3))
        return cls(w[:, :, 0], np.ascontiguousarray(w[:, :, 1]).view(np.float64), np.ascontiguousarray(w[:, :, 2]).view(np.float64), kept0)

    def words(self):
        """-> int64 [G * S * 3], the kernel's layout (the sums as their bits)"""
        G, S = self.counts.shape
        w = np.empty((G, S, 3), np.int64)
        w[:, :, 0], w[:, :, 1], w[:, :, 2] = self.counts, self.esum.view(np.int64), self.ssum.view(np.int64)
        return w.reshape(-1)

    def add(self, other):
        """Accumulate another sample's table: integers add exactly, the sums add in call order.  -> self"""
        if other.counts.shape != self.counts.shape:
            raise ValueError(f"bucket tables of {other.counts.shape} and {self.counts.shape} do not add")
        self.counts = self.counts + other.counts
        self.esum, self.ssum = self.esum + other.esum, self.ssum + other.ssum
        self.kept0 += other.kept0
        return self

    def _rows_sum(self, rows):
        """the rows added in ascending row order -> (counts [S], esum [S], ssum [S])"""
        S = self.counts.shape[1]
        counts, esum, ssum = np.zeros(S, np.int64), np.zeros(S), np.zeros(S)
        for r in sorted(rows):
            counts, esum, ssum = counts + self.counts[r], esum + self.esum[r], ssum + self.ssum[r]
        return counts, esum, ssum

    def meta(self, groups):
        """Rows summed per named group ({name: rows}) in ascending row order; the rows in no group form OTHER, the last
        row.  -> BucketTable of len(groups) + 1 rows with `names`"""
        G = self.counts.shape[0]
        used = [r for rows in groups.values() for r in rows]
        if len(set(used)) != len(used) or any(not 0 <= r < G for r in used):
            raise ValueError("meta: every row belongs to at most one group and lies in the table")
        parts = [self._rows_sum(rows) for rows in groups.values()] + [self._rows_sum(set(range(G)) - set(used))]
        return BucketTable(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
                           self.kept0, tuple(groups) + ("OTHER",))


def bucket_table(args, data, flow_seq, classes=None, speed_edges=ARGO_BUCKET_EDGES, class_lo=ARGO_CLASS_LO, rows=ARGO_CLASS_ROWS):
    """icpflow_seq_bucket_table on one sample -> BucketTable of `rows` class rows (as for class_table) and len(speed_edges) + 1
    speed buckets (|scene_flow| in metres per frame, lower edge inclusive), over the rows calculate_metrics counts.  Inputs as
    for sequence_table; one call, and the one device -> host copy is the table.  There is no CPU path."""
    import ctypes
    import torch
    from . import _lib, utils_loading
    device = utils_loading._device_for(flow_seq, data["raw_points"], data["scene_flow"])
    F = int(args.num_frames)
    raw = data["raw_points"]
    pts = utils_loading.to_device(raw, torch.float64, device)[:, 0:3].contiguous()
    m = pts.shape[0]
    tim = _time_indices(data["time_indice"], F, device)
    cls = utils_loading.to_device(data["classes"] if classes is None else classes, torch.float64, device)
    gt = utils_loading.to_device(data["scene_flow"], torch.float64, device)[:, 0:3].contiguous()
    pred = utils_loading.to_device(flow_seq, torch.float32, device)[:, 0:3].contiguous()
    for name, t in (("time_indice", tim), ("classes", cls), ("scene_flow", gt), ("flow_seq", pred)):
        if t.shape[0] != m or (name == "classes" and t.dim() != 1):
            raise ValueError(f"{name}: {tuple(t.shape)} for {m} points")
    crop, rx, ry, zmin = _crop_arguments(args, raw)
    G = int(rows)
    speed = np.ascontiguousarray(speed_edges, dtype=np.float64).reshape(-1)
    S = len(speed) + 1
    words = G * S * 3
    out = torch.empty(max(words, 0) + 2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_seq_bucket_table_workspace_bytes(m, G, S))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_seq_bucket_table", _lib.ptr(pts), _lib.ptr(tim), _lib.ptr(cls), _lib.ptr(gt), _lib.ptr(pred), m, F, crop, rx, ry,
                  zmin, float(class_lo), G, speed.ctypes.data_as(ctypes.c_void_p) if len(speed) else None, S, _lib.ptr(out),
                  ctypes.c_void_p(out.data_ptr() + words * 8), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    host = out.cpu().numpy()             # the one read-back
    if int(host[words + 1]):
        raise ValueError(f"{int(host[words + 1])} points have a time index outside [0, {F})")
    return BucketTable.from_words(host[:words], G, S, kept0=int(host[words]))


def bucketed_epe(table, groups=ARGO_CHALLENGE_GROUPS):
    """The bucket-normalised EPE over whatever was accumulated.  Per class (the groups, then OTHER = the rows in none):
    `static` = (sum of e) / n of bucket 0, NaN when it is empty; `dynamic` = the plain mean over the non-empty buckets b >= 1 of
    (sum of e)_b / (sum of |gt|)_b -- the bucket's mean EPE over its mean speed -- NaN when there is none; n_static, n_dynamic
    (rows) and buckets_used.  `mean_static` and `mean_dynamic` are the means over the groups' classes, a NaN skipped (NaN when
    every class is NaN); OTHER enters neither.  -> {name: {...} for every class, "mean_static": x, "mean_dynamic": y}"""
    meta = table.meta(groups)
    classes = {}
    with np.errstate(all="ignore"):
        for k, name in enumerate(meta.names):
            n, es, ss = meta.counts[k], meta.esum[k], meta.ssum[k]
            static = float(es[0] / n[0]) if n[0] else float("nan")
            used = [b for b in range(1, len(n)) if n[b]]
            ratios = [float(es[b] / ss[b]) for b in used]
            total = 0.0
            for r in ratios:
                total += r
            dynamic = total / len(ratios) if ratios else float("nan")
            classes[name] = dict(static=static, dynamic=float(dynamic), n_static=int(n[0]), n_dynamic=int(n[1:].sum()), buckets_used=len(used))

    def mean(key):
        total, k = 0.0, 0
        for name in groups:
            v = classes[name][key]
            if v == v:
                total, k = total + v, k + 1
        return total / k if k else float("nan")

    return dict(classes, mean_static=mean("static"), mean_dynamic=mean("dynamic"))


def format_bucketed_epe(result):
    """bucketed_epe's dict as lines: one per class, then the two means."""
    text = ["################# Bucket-normalised EPE per class #####################################"]
    for name, c in result.items():
        if not isinstance(c, dict):
            continue
        text.append(f"{name:>16}, static EPE: {c['static']:.6f} (n {c['n_static']}), dynamic normalised EPE: {c['dynamic']:.6f} "
                    f"(n {c['n_dynamic']}, {c['buckets_used']} buckets)")
    text.append(f"mean static EPE: {result['mean_static']:.6f}, mean dynamic normalised EPE: {result['mean_dynamic']:.6f}")
    return "\n".join(text)


def save_metrics_file(path, metrics_per_frame, num_frames):
    """The reference's closing file (main.py:298-312, np.savez): per meter <name> of the table the keys EPE3D<name> -- no
    underscore, as the reference writes it -- ACC3DS_<name>, ACC3DR_<name>, OUTLIER_<name> and ROUTLIER_<name>, each the
    meter's `*_data` list as an array of shape [1, n] (what the reference's trailing commas make of the lists).  -> the keys"""
    prefixes = ("EPE3D", "ACC3DS_", "ACC3DR_", "OUTLIER_", "ROUTLIER_")
    out = {}
    for k in range(0, num_frames + 1):
        for metric in METRIC_CLASSES:
            name = metric + f"_{k:d}"
            for prefix, field in zip(prefixes, METRIC_NAMES):
                out[prefix + name] = np.asarray(getattr(metrics_per_frame[name], field + "_data"), dtype=np.float64).reshape(1, -1)
    with open(path, "wb") as f:           # (np.savez would append ".npz" to a name without it)
        np.savez(f, **out)
    return list(out)


# ---- judged without ground truth: the truncated nearest-neighbour residual (icpflow_nn_residual, csrc/nnresid.hip) ----------
RESIDUAL_EDGES = (0.05, 0.1)           # metres: the reference's AccS / AccR distances (utils_eval.py:65-182)
RESIDUAL_GROUPS = ("ground", "unclustered", "unmatched", "matched")   # run_stream's groups of the source rows


class ResidualTable:
    """icpflow_nn_residual's table on the host, per group of query rows: rows int64 [G] (good rows), hits int64 [G] (rows with
    a neighbour within the radius), under int64 [G,E] (rows with d <= edge), dsum and ddsum float64 [G] (sums of d and of d * d,
    d truncated at the radius); edges (metres), radius, bad (rows the call refused: bad coordinates or group)."""

    def __init__(self, rows, hits, under, dsum, ddsum, edges=(), radius=None, bad=0):
        self.rows, self.hits = np.array(rows, dtype=np.int64).reshape(-1), np.array(hits, dtype=np.int64).reshape(-1)
        G = len(self.rows)
        self.edges = tuple(float(e) for e in edges)
        self.under = np.array(under, dtype=np.int64).reshape(G, len(self.edges))
        self.dsum, self.ddsum = np.array(dsum, dtype=np.float64).reshape(-1), np.array(ddsum, dtype=np.float64).reshape(-1)
        self.radius = None if radius is None else float(radius)
        self.bad = int(bad)
        assert len(self.hits) == G and len(self.dsum) == G and len(self.ddsum) == G

    @classmethod
    def zeros(cls, G, edges=RESIDUAL_EDGES, radius=None):
        return cls(np.zeros(G, np.int64), np.zeros(G, np.int64), np.zeros((G, len(edges)), np.int64), np.zeros(G), np.zeros(G), edges, radius)

    @classmethod
    def from_words(cls, words, G, edges=RESIDUAL_EDGES, radius=None, bad=0):
        """the kernel's int64 [G][E + 4] -> ResidualTable"""
        E = len(edges)
        w = np.ascontiguousarray(np.asarray(words, dtype=np.int64).reshape(G, E + 4))
        return cls(w[:, 0], w[:, 1], w[:, 2:2 + E], np.ascontiguousarray(w[:, 2 + E]).view(np.float64),
                   np.ascontiguousarray(w[:, 3 + E]).view(np.float64), edges, radius, bad)

    def words(self):
        """-> int64 [G * (E + 4)], the kernel's layout (the sums as their bits)"""
        G, E = len(self.rows), len(self.edges)
        w = np.empty((G, E + 4), np.int64)
        w[:, 0], w[:, 1], w[:, 2:2 + E] = self.rows, self.hits, self.under
        w[:, 2 + E], w[:, 3 + E] = self.dsum.view(np.int64), self.ddsum.view(np.int64)
        return w.reshape(-1)

    def add(self, other):
        """Accumulate another call's table: integers add exactly, the sums add in call order.  -> self"""
        if other.under.shape != self.under.shape or other.edges != self.edges:
            raise ValueError(f"residual tables of {other.under.shape} {other.edges} and {self.under.shape} {self.edges} do not add")
        self.rows, self.hits, self.under = self.rows + other.rows, self.hits + other.hits, self.under + other.under
        self.dsum, self.ddsum = self.dsum + other.dsum, self.ddsum + other.ddsum
        self.bad += other.bad
        return self

    def _pick(self, v, group):
        """one group's value, or (group None) the groups' values added in ascending order"""
        if group is not None:
            return v[group]
        total = v[0] * 0
        for g in range(len(v)):
            total = total + v[g]
        return total

    def n(self, group=None):
        return int(self._pick(self.rows, group))

    def hit_rate(self, group=None):
        n = self.n(group)
        return float(self._pick(self.hits, group)) / n if n else float("nan")

    def mean(self, group=None):
        """the mean truncated distance in metres (NaN for an empty group)"""
        n = self.n(group)
        return float(self._pick(self.dsum, group)) / n if n else float("nan")

    def rms(self, group=None):
        n = self.n(group)
        return float(np.sqrt(float(self._pick(self.ddsum, group)) / n)) if n else float("nan")

    def shares(self, group=None):
        """per edge the share of the rows with d <= edge"""
        n = self.n(group)
        under = self._pick(self.under, group)
        return tuple(float(u) / n if n else float("nan") for u in under)

    def summary(self, names=None):
        """-> JSON-ready: the whole table and one entry per group"""
        def entry(g):
            return dict(n=self.n(g), hit_rate=self.hit_rate(g), mean=self.mean(g), rms=self.rms(g), shares=list(self.shares(g)))
        G = len(self.rows)
        names = list(names) if names is not None else [str(g) for g in range(G)]
        return dict(all=entry(None), groups={names[g]: entry(g) for g in range(G)}, bad_rows=self.bad)


def _cloud3(t, name):
    import torch
    from . import _lib
    _lib.require_gpu(t)
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"{name}: expected [n, 3], got {tuple(t.shape)}")
    return t[:, 0:3].to(torch.float32).contiguous()


def nn_residual_device(query, target, flow=None, radius=2.0, groups=None, n_groups=1, edges=RESIDUAL_EDGES, per_row=True):
    """icpflow_nn_residual enqueued on the current stream, nothing read back.  -> (d2 float32 [n], idx int32 [n], words): words is
    an int64 device tensor [n_groups * (len(edges) + 4) + 4], the table followed by d_info (bad queries, bad targets, occupied
    buckets, longest bucket).  per_row False: d2 and idx are None (the call keeps them in its workspace)."""
    import ctypes
    import torch
    from . import _lib
    q, t = _cloud3(query, "query"), _cloud3(target, "target")
    device = q.device
    n, m, G = q.shape[0], t.shape[0], int(n_groups)
    f = g = None
    if flow is not None:
        f = _cloud3(flow, "flow")
        if f.shape[0] != n:
            raise ValueError(f"flow: {tuple(f.shape)} for {n} query rows")
    if groups is not None:
        _lib.require_gpu(groups)
        g = groups.to(torch.int32).contiguous()
        if g.shape != (n,):
            raise ValueError(f"groups: {tuple(g.shape)} for {n} query rows")
    if t.device != device or (f is not None and f.device != device) or (g is not None and g.device != device):
        raise ValueError("nn_residual: every tensor on the same device")
    ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    E = len(ed)
    words = max(G, 0) * (E + 4)
    out = torch.empty(words + 4, dtype=torch.int64, device=device)
    d2 = torch.empty(n, dtype=torch.float32, device=device) if per_row else None
    idx = torch.empty(n, dtype=torch.int32, device=device) if per_row else None
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_nn_residual_workspace_bytes(n, m, G, E))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_nn_residual", _lib.ptr(q), _lib.ptr(f), n, _lib.ptr(t), m, float(radius), _lib.ptr(g), G,
                  ed.ctypes.data_as(ctypes.c_void_p) if E else None, E, _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(out),
                  ctypes.c_void_p(out.data_ptr() + words * 8), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return d2, idx, out


def nn_residual(query, target, flow=None, radius=2.0, groups=None, n_groups=1, edges=RESIDUAL_EDGES):
    """The truncated nearest-neighbour residual of `query` (+ `flow`) against `target`: per query row the squared distance to
    the nearest target within `radius` metres (radius^2 without one) and that target's row (-1 without one, -2 for a bad row:
    non-finite, beyond 1e6 m, or a group outside [0, n_groups)), and the table per group of rows (`groups` int [n], None: one
    group).  float32 [n,3] tensors on the GPU; there is no CPU path.  -> (d2 float32 [n], idx int32 [n], ResidualTable); one
    small read-back, the table."""
    d2, idx, out = nn_residual_device(query, target, flow, radius, groups, n_groups, edges)
    host = out.cpu().numpy()
    words = len(host) - 4
    table = ResidualTable.from_words(host[:words], int(n_groups), tuple(float(e) for e in edges), radius, bad=int(host[words]))
    table.info = dict(bad_queries=int(host[words]), bad_targets=int(host[words + 1]), occupied_buckets=int(host[words + 2]),
                      longest_bucket=int(host[words + 3]))
    return d2, idx, table


def chamfer(a, b, radius=2.0, edges=RESIDUAL_EDGES):
    """The truncated Chamfer distance of two clouds through two calls: a against b, b against a.  -> dict(forward, backward:
    ResidualTable, chamfer: the sum of the two mean truncated distances in metres)"""
    _, _, fwd = nn_residual(a, b, radius=radius, edges=edges)
    _, _, bwd = nn_residual(b, a, radius=radius, edges=edges)
    return dict(forward=fwd, backward=bwd, chamfer=fwd.mean() + bwd.mean())


def format_residual(before, after, names=RESIDUAL_GROUPS):
    """The residual lines of a run.  `before` and `after`: dict(forward, backward: ResidualTable) -- the source under the ego
    pose alone and under the predicted flow against the destination, and the destination against either."""
    fb, fa = before["forward"], after["forward"]
    text = [f"################# Nearest-neighbour residual, truncated at {fa.radius:g} m (no ground truth) ##############"]

    def line(name, g):
        shares = ", ".join(f"<= {e:g} m: {b:.4f} -> {a:.4f}" for e, b, a in zip(fa.edges, fb.shares(g), fa.shares(g)))
        return (f"{name:>12}, n {fa.n(g)}, mean: {fb.mean(g):.6f} -> {fa.mean(g):.6f}, rms: {fb.rms(g):.6f} -> {fa.rms(g):.6f}, "
                f"hit rate: {fb.hit_rate(g):.4f} -> {fa.hit_rate(g):.4f}" + (", " + shares if shares else ""))

    for g in range(len(fa.rows)):
        text.append(line(names[g] if names is not None and g < len(names) else str(g), g))
    text.append(line("all", None))
    cb, ca = fb.mean() + before["backward"].mean(), fa.mean() + after["backward"].mean()
    text.append(f"truncated Chamfer distance (source -> destination + destination -> source): {cb:.6f} -> {ca:.6f}")
    return "\n".join(text)


# ---- ... per segment, before and after the flow (icpflow_nn_residual_segments, csrc/segresid.hip) -----------------------------
RESIDUAL_SKIP_LABELS = (-1e8, -1.0)    # the ground and the unclustered rows: segments no registration moved


class SegmentResidual:
    """icpflow_nn_residual_segments' table on the host: labels float64 [L] ascending, rows int64 [L] (rows of the segment, the
    bad ones included), and per side -- `before`: the ego-compensated source, `after`: the cloud under the predicted flow, both
    against the destination -- a ResidualTable with one group per segment; info: the call's d_info."""

    def __init__(self, labels, rows, before, after, info=None):
        self.labels, self.rows = np.array(labels, dtype=np.float64).reshape(-1), np.array(rows, dtype=np.int64).reshape(-1)
        self.before, self.after = before, after
        self.info = dict(info or {})
        assert len(self.rows) == len(self.labels) == len(before.rows) == len(after.rows)

    @classmethod
    def from_table(cls, table, edges=RESIDUAL_EDGES, radius=None, info=None):
        """the kernel's float64 [L][18] -> SegmentResidual"""
        t = np.asarray(table, dtype=np.float64).reshape(-1, 18)
        E = len(edges)
        info = dict(info or {})

        def side(at, bad):
            return ResidualTable(np.rint(t[:, at]), np.rint(t[:, at + 1]), np.rint(t[:, at + 2: at + 2 + E]), t[:, at + 6], t[:, at + 7],
                                 edges, radius, bad)

        return cls(t[:, 0], np.rint(t[:, 1]), side(2, info.get("bad_queries_before", 0)), side(10, info.get("bad_queries_after", 0)), info)

    def __len__(self):
        return len(self.labels)

    def gain(self):
        """per segment the mean truncated distance the flow took away, in metres: before.mean - after.mean (negative: the flow
        made the segment fit worse; NaN for a segment without a good row on either side)"""
        return np.array([self.before.mean(k) - self.after.mean(k) for k in range(len(self))], dtype=np.float64)

    def worst(self, pairs=None, above=RESIDUAL_EDGES[1], skip=RESIDUAL_SKIP_LABELS):
        """The segments whose AFTER mean exceeds `above` metres, worst first, equal means by ascending label; the labels of
        `skip` are left out.  pairs ([P, >= 2], column 0 the source label, column 1 the destination's): `matched` says whether
        the segment is a source of one, `pair` is that row's [src, dst] (None without one).  -> [dict(label, rows, after_mean,
        before_mean, gain, hit_rate_after, matched, pair)]"""
        by_src = {}
        if pairs is not None:
            p = pairs.detach().cpu().numpy() if hasattr(pairs, "detach") else np.asarray(pairs)
            for row in np.asarray(p, dtype=np.float64).reshape(len(p), -1):
                by_src.setdefault(float(row[0]), [float(row[0]), float(row[1])])
        left_out = set(float(s) for s in skip)
        out = []
        for k in range(len(self)):
            label, after = float(self.labels[k]), self.after.mean(k)
            if label in left_out or not after > above:       # (a NaN mean -- no good row -- is not listed)
                continue
            before = self.before.mean(k)
            out.append(dict(label=label, rows=int(self.rows[k]), after_mean=after, before_mean=before, gain=before - after,
                            hit_rate_after=self.after.hit_rate(k), matched=label in by_src, pair=by_src.get(label)))
        return sorted(out, key=lambda e: (-e["after_mean"], e["label"]))


def segment_residual_device(before, after, flow, labels, target, radius=2.0, edges=RESIDUAL_EDGES, Lmax=4096, per_row=False):
    """icpflow_nn_residual_segments enqueued on the current stream, nothing read back.  before, after [n, 3], flow [n, 3] or None,
    labels [n], target [m, 3]: device tensors (`after` may be `before`).  -> (table float64 [Lmax, 18], num int32 [1], info
    int64 [6], d2_before, d2_after): device tensors; the last two float32 [n] with per_row, else None (the call keeps them in
    its workspace).  Rows of the table from num on are not written."""
    import ctypes
    import torch
    from . import _lib
    b, t = _cloud3(before, "before"), _cloud3(target, "target")
    a = b if after is before else _cloud3(after, "after")
    device = b.device
    n, m, Lmax = b.shape[0], t.shape[0], int(Lmax)
    f = None
    if flow is not None:
        f = _cloud3(flow, "flow")
    _lib.require_gpu(labels)
    lab = labels.to(torch.float32).contiguous()
    if a.shape[0] != n or (f is not None and f.shape[0] != n) or lab.shape != (n,):
        raise ValueError(f"segment_residual: after {tuple(a.shape)}, flow {None if f is None else tuple(f.shape)}, labels {tuple(lab.shape)} for {n} rows")
    if any(x is not None and x.device != device for x in (a, f, lab, t)):
        raise ValueError("segment_residual: every tensor on the same device")
    ed = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    E = len(ed)
    table = torch.empty((max(Lmax, 0), _lib.NNRS_COLS), dtype=torch.float64, device=device)
    num = torch.empty(1, dtype=torch.int32, device=device)
    info = torch.empty(6, dtype=torch.int64, device=device)
    d2b = torch.empty(n, dtype=torch.float32, device=device) if per_row else None
    d2a = torch.empty(n, dtype=torch.float32, device=device) if per_row else None
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_nn_residual_segments_workspace_bytes(n, m, Lmax, E))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_nn_residual_segments", _lib.ptr(b), _lib.ptr(a), _lib.ptr(f), _lib.ptr(lab), n, _lib.ptr(t), m, float(radius),
                  ed.ctypes.data_as(ctypes.c_void_p) if E else None, E, _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(d2b), _lib.ptr(d2a),
                  _lib.ptr(info), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return table, num, info, d2b, d2a


SEGMENT_INFO_NAMES = ("bad_queries_before", "bad_queries_after", "bad_targets", "occupied_buckets", "longest_bucket")


def segment_residual(before, after, flow, labels, target, radius=2.0, edges=RESIDUAL_EDGES, Lmax=4096):
    """The truncated nearest-neighbour residual of every segment (distinct label) of a source cloud against `target`, BEFORE
    (`before` as it is) and AFTER (`after` + `flow`): one grid over the target, two queries, one table.  Tensors on the GPU;
    there is no CPU path.  -> SegmentResidual; one read-back (the table, the number of segments and the info in one tensor).
    More distinct labels than Lmax is a ValueError."""
    table, num, info, _, _ = segment_residual_device(before, after, flow, labels, target, radius, edges, Lmax)
    return segment_residual_read(table, num, info, radius, edges)


def segment_residual_read(table, num, info, radius=2.0, edges=RESIDUAL_EDGES):
    """segment_residual_device's table, number of segments and info read back in one tensor.  -> SegmentResidual"""
    import torch
    host = torch.cat([num.to(torch.float64), info.to(torch.float64), table.reshape(-1)]).cpu().numpy()     # the one read-back
    L = int(host[0])
    if L < 0:
        raise ValueError(f"segment_residual: {-L} distinct labels, Lmax = {int(table.shape[0])}")
    facts = {name: int(host[1 + k]) for k, name in enumerate(SEGMENT_INFO_NAMES)}
    return SegmentResidual.from_table(host[7: 7 + L * 18], tuple(float(e) for e in edges), radius, facts)


def format_segment_residual(report):
    """One line per listed segment (SegmentResidual.worst's entries, or run_stream's, which carry `frame_pair` too), in the
    shape of flow_evaluation's `eval segment:` line."""
    lines = []
    for e in report:
        where = f"frame pair: {e['frame_pair']:4d}, " if "frame_pair" in e else ""
        pair = e.get("pair")
        ij = f"i: {int(pair[0]):3d}, j: {int(pair[1]):3d}" if pair else "unmatched"
        lines.append(f"residual segment: {where}{e['label']:3g}, after: {e['after_mean']:.4f}, before: {e['before_mean']:.4f}, "
                     f"gain: {e['gain']:.4f}, {ij}; len_i: {e['rows']:6d}, hit rate: {e['hit_rate_after']:.4f}")
    return lines


# ---- line of sight: a missing neighbour told apart (icpflow_sight_*, csrc/sight.hip) -------------------------------------------
SIGHT_VERDICTS = ("seen through", "lost from view", "undecided")
SIGHT_EXCUSED = (0, 1, 4)              # outside the field of view, on a ray without a return, behind the first return


class SightImage:
    """The depth image of one destination sweep on the device (icpflow_sight_build): image uint32 [2, H, W] -- plane 0 the bits
    of the nearest range per pixel, plane 1 its minimum over the 3 x 3 pixels around --, the parameters it was built with
    (_lib.SightParams), the sensor origin (float64 [3]) and info, int64 [3] on the device: bad targets, targets outside the
    field of view, occupied pixels."""

    def __init__(self, image, params, origin, info):
        self.image, self.params, self.info = image, params, info
        self.origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)

    @property
    def device(self):
        return self.image.device

    def _args(self):
        import ctypes
        from . import _lib
        return _lib.ptr(self.image), ctypes.byref(self.params), self.origin.ctypes.data_as(ctypes.c_void_p)


def sight_image(points_dst, origin=(0.0, 0.0, 0.0), **params):
    """The depth image of the destination sweep `points_dst` ([m, 3] on the GPU; there is no CPU path) as seen from `origin`
    -- the sensor's position in the frame of the points --, enqueued on the current stream.  params: fields of
    icpflow_sight_params_t (W, H, tan_lo, tan_hi, min_range, max_range, margin_abs, margin_rel) that replace the library's
    defaults.  -> SightImage"""
    import ctypes
    import torch
    from . import _lib
    t = _cloud3(points_dst, "points_dst")
    p = _lib.SightParams.defaults(**params)
    o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    image = torch.empty((2, max(int(p.H), 0), max(int(p.W), 0)), dtype=torch.int32, device=t.device)   # (the bits of a uint32 image)
    info = torch.empty(3, dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        _lib.call("icpflow_sight_build", _lib.ptr(t), t.shape[0], o.ctypes.data_as(ctypes.c_void_p), ctypes.byref(p), _lib.ptr(image),
                  _lib.ptr(info), _lib.stream(t.device))
    return SightImage(image, p, o, info)


def line_of_sight(image, points, flow=None, near=False):
    """The ray test of every row of `points` (+ `flow`) against a SightImage, enqueued on the current stream: -> codes int32 [n]
    on the device (-2 a bad row, 0 outside the field of view, 1 no return on the ray, 2 seen through, 3 at the first return,
    4 behind it); with near=True -> (codes, near float32 [n]: the nearest range of the 3 x 3 pixels, +inf without a pixel).
    The six counts stay on the device as `image.last_counts` (int64 [6]: bad rows, then codes 0 .. 4)."""
    import torch
    from . import _lib
    q = _cloud3(points, "points")
    f = None if flow is None else _cloud3(flow, "flow")
    n = q.shape[0]
    if f is not None and f.shape[0] != n:
        raise ValueError(f"flow: {tuple(f.shape)} for {n} rows")
    if q.device != image.device or (f is not None and f.device != image.device):
        raise ValueError("line_of_sight: every tensor on the image's device")
    codes = torch.empty(n, dtype=torch.int32, device=q.device)
    nearest = torch.empty(n, dtype=torch.float32, device=q.device) if near else None
    counts = torch.empty(6, dtype=torch.int64, device=q.device)
    with torch.cuda.device(q.device):
        _lib.call("icpflow_sight_query", *image._args(), _lib.ptr(q), _lib.ptr(f), n, _lib.ptr(codes), _lib.ptr(nearest), _lib.ptr(counts),
                  _lib.stream(q.device))
    image.last_counts = counts
    return (codes, nearest) if near else codes


class SightCounts:
    """one side of icpflow_sight_segments' table: good int64 [L], codes int64 [L, 5] (the rows of codes 0 .. 4), far int64
    [L, 5] (the FAR rows among them)"""

    def __init__(self, good, codes, far):
        self.good = np.array(good, dtype=np.int64).reshape(-1)
        self.codes, self.far = np.array(codes, dtype=np.int64).reshape(-1, 5), np.array(far, dtype=np.int64).reshape(-1, 5)


class SegmentSight:
    """icpflow_sight_segments' table on the host: labels float64 [L] ascending, rows int64 [L], `before` and `after`
    SightCounts; info: the twelve counts of the call (bad rows and codes 0 .. 4 of either side)."""

    def __init__(self, labels, rows, before, after, info=None):
        self.labels, self.rows = np.array(labels, dtype=np.float64).reshape(-1), np.array(rows, dtype=np.int64).reshape(-1)
        self.before, self.after = before, after
        self.info = dict(info or {})
        assert len(self.rows) == len(self.labels) == len(before.good) == len(after.good)

    @classmethod
    def from_table(cls, table, info=None):
        """the kernel's float64 [L][24] -> SegmentSight"""
        t = np.rint(np.asarray(table, dtype=np.float64).reshape(-1, 24))
        side = lambda at: SightCounts(t[:, at], t[:, at + 1: at + 11: 2], t[:, at + 2: at + 12: 2])   # noqa: E731
        return cls(np.asarray(table, dtype=np.float64).reshape(-1, 24)[:, 0], t[:, 1], side(2), side(13), info)

    def __len__(self):
        return len(self.labels)

    def far_rows(self, k):
        """the good rows of segment k under the flow that are FAR from every destination point"""
        return int(self.after.far[k].sum())

    def seen_through_share(self, k):
        """among the FAR rows of segment k under the flow, the share the destination sweep saw through (NaN without a far row)"""
        n = self.far_rows(k)
        return float(self.after.far[k, 2]) / n if n else float("nan")

    def excused_share(self, k):
        """... the share that is merely unobserved: outside the field of view, no return on the ray, or behind the first return"""
        n = self.far_rows(k)
        return float(sum(int(self.after.far[k, c]) for c in SIGHT_EXCUSED)) / n if n else float("nan")

    def annotate(self, entries, share=0.5):
        """SegmentResidual.worst's entries (dicts with a `label`) with `seen_through`, `excused` and `far_rows` (rows) and a
        `verdict` added to each: "seen through" when more than `share` of the far rows have code 2, "lost from view" when more
        than `share` have codes 0, 1 or 4, else "undecided" (a tie, a majority at the first return, or no far row).  -> entries"""
        at = {float(v): k for k, v in enumerate(self.labels.tolist())}
        for e in entries:
            k = at.get(float(e["label"]))
            if k is None:
                raise ValueError(f"annotate: no segment with label {e['label']!r}")
            far = self.far_rows(k)
            seen, excused = int(self.after.far[k, 2]), int(sum(int(self.after.far[k, c]) for c in SIGHT_EXCUSED))
            verdict = "seen through" if seen > share * far else "lost from view" if excused > share * far else "undecided"
            e.update(seen_through=seen, excused=excused, far_rows=far, verdict=verdict)
        return entries


def segment_sight_device(image, before, after, flow, labels, d2_before=None, d2_after=None, far=RESIDUAL_EDGES[1], Lmax=4096, per_row=False):
    """icpflow_sight_segments enqueued on the current stream, nothing read back.  image: a SightImage; before, after [n, 3], flow
    [n, 3] or None, labels [n]; d2_before, d2_after: float32 [n] as segment_residual_device(per_row=True) returns them, or None
    (then no row is FAR).  -> (table float64 [Lmax, 24], num int32 [1], info int64 [12], code_before, code_after): device
    tensors; the last two int32 [n] with per_row, else None."""
    import ctypes
    import torch
    from . import _lib
    b = _cloud3(before, "before")
    a = b if after is before else _cloud3(after, "after")
    device = b.device
    n, Lmax = b.shape[0], int(Lmax)
    f = None if flow is None else _cloud3(flow, "flow")
    _lib.require_gpu(labels, d2_before, d2_after)
    lab = labels.to(torch.float32).contiguous()
    d2 = [None if d is None else d.to(torch.float32).contiguous() for d in (d2_before, d2_after)]
    if a.shape[0] != n or (f is not None and f.shape[0] != n) or lab.shape != (n,) or any(d is not None and d.shape != (n,) for d in d2):
        raise ValueError(f"segment_sight: after {tuple(a.shape)}, flow {None if f is None else tuple(f.shape)}, labels {tuple(lab.shape)} for {n} rows")
    if any(x is not None and x.device != device for x in (a, f, lab, image.image, *d2)):
        raise ValueError("segment_sight: every tensor on the same device")
    table = torch.empty((max(Lmax, 0), _lib.SIGHT_COLS), dtype=torch.float64, device=device)
    num = torch.empty(1, dtype=torch.int32, device=device)
    info = torch.empty(12, dtype=torch.int64, device=device)
    codes = [torch.empty(n, dtype=torch.int32, device=device) if per_row else None for _ in range(2)]
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_sight_segments_workspace_bytes(n, Lmax))
        ws = _lib.workspace(device, need)
        _lib.call("icpflow_sight_segments", *image._args(), _lib.ptr(b), _lib.ptr(a), _lib.ptr(f), _lib.ptr(lab), n, _lib.ptr(d2[0]), _lib.ptr(d2[1]),
                  float(far), _lib.ptr(table), Lmax, _lib.ptr(num), _lib.ptr(codes[0]), _lib.ptr(codes[1]), _lib.ptr(info), _lib.ptr(ws),
                  ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return table, num, info, codes[0], codes[1]


SIGHT_INFO_NAMES = tuple(f"{side}_{name}" for side in ("before", "after")
                         for name in ("bad_rows", "outside", "no_return", "seen_through", "at_first_return", "behind"))


def segment_sight(image, before, after, flow, labels, d2_before=None, d2_after=None, far=RESIDUAL_EDGES[1], Lmax=4096):
    """The line-of-sight codes of every segment (distinct label) of a source cloud against the SightImage of the destination,
    BEFORE (`before` as it is) and AFTER (`after` + `flow`), and among them the rows whose nearest destination point is more
    than `far` metres away.  Tensors on the GPU; there is no CPU path.  -> SegmentSight; one read-back.  More distinct labels
    than Lmax is a ValueError."""
    import torch
    table, num, info, _, _ = segment_sight_device(image, before, after, flow, labels, d2_before, d2_after, far, Lmax)
    host = torch.cat([num.to(torch.float64), info.to(torch.float64), table.reshape(-1)]).cpu().numpy()     # the one read-back
    L = int(host[0])
    if L < 0:
        raise ValueError(f"segment_sight: {-L} distinct labels, Lmax = {int(Lmax)}")
    facts = {name: int(host[1 + k]) for k, name in enumerate(SIGHT_INFO_NAMES)}
    return SegmentSight.from_table(host[13: 13 + L * 24], facts)


def format_segment_sight(report):
    """One line per listed segment that SegmentSight.annotate has been through, behind format_segment_residual's line."""
    lines = []
    for line, e in zip(format_segment_residual(report), report):
        lines.append(f"{line}; far rows: {e['far_rows']:6d}, seen through: {e['seen_through']:6d}, excused: {e['excused']:6d}, {e['verdict']}")
    return lines


# ---- the trust byte: the two verdicts per source point (icpflow_flow_trust, csrc/trust.hip) ------------------------------------
TRUST_ROW_MASK, TRUST_FIT_SHIFT, TRUST_FIT_MASK = 0x07, 3, 0x03
TRUST_MATCHED, TRUST_SKIPPED, TRUST_KEEP = 0x20, 0x40, 0x80
TRUST_ROW_NAMES = ("not_judged", "near", "seen_through", "at_first_return", "behind", "no_return", "outside", "far_no_code")
TRUST_FIT_NAMES = ("fits", "seen_through", "lost_from_view", "undecided")


class TrustCounts:
    """icpflow_flow_trust's d_counts on the host: rows int64 [8] (the rows with a segment per ROW class, TRUST_ROW_NAMES), fit
    int64 [4] (the judged rows of segments that are not skipped per FIT class, TRUST_FIT_NAMES), matched, skipped, kept (the
    rows with bit 5, 6, 7) and no_segment (the rows whose label has no segment: byte 0)."""

    def __init__(self, words=None):
        w = np.zeros(16, np.int64) if words is None else np.array(words, dtype=np.int64).reshape(16)
        self.rows, self.fit = w[0:8].copy(), w[8:12].copy()
        self.matched, self.skipped, self.kept, self.no_segment = int(w[12]), int(w[13]), int(w[14]), int(w[15])

    def words(self):
        """-> int64 [16], the kernel's layout"""
        return np.concatenate([self.rows, self.fit, [self.matched, self.skipped, self.kept, self.no_segment]]).astype(np.int64)

    def add(self, other):
        """Accumulate another call's counts (integers: exact in any order).  -> self"""
        self.rows, self.fit = self.rows + other.rows, self.fit + other.fit
        self.matched, self.skipped = self.matched + other.matched, self.skipped + other.skipped
        self.kept, self.no_segment = self.kept + other.kept, self.no_segment + other.no_segment
        return self

    def n(self):
        """every row the calls saw"""
        return int(self.rows.sum()) + self.no_segment

    def kept_share(self):
        """the share of all rows with KEEP set (NaN without a row)"""
        n = self.n()
        return self.kept / n if n else float("nan")

    def summary(self):
        """-> JSON-ready"""
        return dict(n=self.n(), rows=dict(zip(TRUST_ROW_NAMES, self.rows.tolist())), fit=dict(zip(TRUST_FIT_NAMES, self.fit.tolist())),
                    matched=self.matched, skipped=self.skipped, kept=self.kept, no_segment=self.no_segment, kept_share=self.kept_share())


def flow_trust_device(after, flow, labels, resid_table, num, d2_after, pairs=None, sight_table=None, code_after=None, params=None):
    """icpflow_flow_trust enqueued on the current stream, nothing read back.  after [n, 3], flow [n, 3] or None, labels [n]: what
    segment_residual_device took; resid_table, num, d2_after: what it returned (per_row=True); sight_table, code_after: what
    segment_sight_device returned for the same cloud (per_row=True), or both None; pairs [P, >= 1] (column 0 the source label
    of a matched pair, as the registration leaves them) or None; params: a _lib.TrustParams (None: the library's defaults).
    Device tensors; there is no CPU path.  -> (trust uint8 [n], segment uint8 [Lmax], counts int64 [16]) on the device; bytes of
    `segment` from num on are not written."""
    import ctypes
    import torch
    from . import _lib
    a = _cloud3(after, "after")
    device = a.device
    n = a.shape[0]
    f = None if flow is None else _cloud3(flow, "flow")
    _lib.require_gpu(labels, resid_table, num, d2_after, pairs, sight_table, code_after)
    lab, d2 = labels.to(torch.float32).contiguous(), d2_after.to(torch.float32).contiguous()
    if resid_table.dtype != torch.float64 or resid_table.dim() != 2 or resid_table.shape[1] != _lib.NNRS_COLS or not resid_table.is_contiguous():
        raise ValueError(f"flow_trust: resid_table {tuple(resid_table.shape)} {resid_table.dtype}, expected contiguous float64 [Lmax, {_lib.NNRS_COLS}]")
    Lmax = int(resid_table.shape[0])
    if sight_table is not None and (sight_table.dtype != torch.float64 or tuple(sight_table.shape) != (Lmax, _lib.SIGHT_COLS) or not sight_table.is_contiguous()):
        raise ValueError(f"flow_trust: sight_table {tuple(sight_table.shape)} {sight_table.dtype}, expected contiguous float64 [{Lmax}, {_lib.SIGHT_COLS}]")
    if (sight_table is None) != (code_after is None):
        raise ValueError("flow_trust: the sight table and the per-row codes come together or not at all")
    code = None if code_after is None else code_after.to(torch.int32).contiguous()
    if num.dtype != torch.int32 or num.numel() != 1:
        raise ValueError(f"flow_trust: num {tuple(num.shape)} {num.dtype}, expected int32 [1]")
    if (f is not None and f.shape[0] != n) or lab.shape != (n,) or d2.shape != (n,) or (code is not None and code.shape != (n,)):
        raise ValueError(f"flow_trust: flow {None if f is None else tuple(f.shape)}, labels {tuple(lab.shape)}, d2_after {tuple(d2.shape)}, "
                         f"code_after {None if code is None else tuple(code.shape)} for {n} rows")
    rows, P, stride = None, 0, 1
    if pairs is not None and pairs.shape[0] > 0:
        if pairs.dim() != 2 or pairs.shape[1] < 1:
            raise ValueError(f"flow_trust: pairs {tuple(pairs.shape)}, expected [P, >= 1]")
        rows = pairs.to(torch.float32).contiguous()
        P, stride = int(rows.shape[0]), int(rows.shape[1])
    if any(x is not None and x.device != device for x in (f, lab, d2, code, resid_table, sight_table, num, rows)):
        raise ValueError("flow_trust: every tensor on the same device")
    p = params if params is not None else _lib.TrustParams.defaults()
    trust = torch.empty(n, dtype=torch.uint8, device=device)
    segment = torch.empty(Lmax, dtype=torch.uint8, device=device)
    counts = torch.empty(_lib.TRUST_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.call("icpflow_flow_trust", _lib.ptr(a), _lib.ptr(f), _lib.ptr(lab), n, _lib.ptr(resid_table), _lib.ptr(sight_table), _lib.ptr(num), Lmax,
                  _lib.ptr(d2), _lib.ptr(code), _lib.ptr(rows), P, stride, ctypes.byref(p), _lib.ptr(trust), _lib.ptr(segment), _lib.ptr(counts),
                  _lib.stream(device))
    return trust, segment, counts


def flow_trust(after, flow, labels, resid_table, num, d2_after, pairs=None, sight_table=None, code_after=None, params=None):
    """One trust byte per row of a source cloud from the tables and per-row arrays of segment_residual_device and (optionally)
    segment_sight_device: bits 0-2 the row's class (TRUST_ROW_NAMES), bits 3-4 its segment's fit (TRUST_FIT_NAMES), TRUST_MATCHED,
    TRUST_SKIPPED, TRUST_KEEP (include/icpflow_hip.h, 8(i)).  Tensors on the GPU; there is no CPU path.  -> (trust uint8 [n] on
    the device, TrustCounts); one read-back of sixteen words."""
    trust, _, counts = flow_trust_device(after, flow, labels, resid_table, num, d2_after, pairs, sight_table, code_after, params)
    return trust, TrustCounts(counts.cpu().numpy())


def trust_keep(trust):
    """the rows to keep as pseudo labels: bit 7 of the trust byte (a torch tensor or a numpy array of uint8) -> bool, same kind"""
    return (trust & TRUST_KEEP) != 0

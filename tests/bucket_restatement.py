"""A plain fp64 numpy restatement of icpflow_seq_bucket_table (include/icpflow_hip.h) and of the bucket-normalised EPE of the
Argoverse 2 2024 challenge (Khatri et al., "I Can't Believe It's Not Scene Flow!", ECCV 2024), written from their definitions:
the pass keeps, per (class row, speed bucket), the rows' e and |gt| as lists in row order; the metric is computed from exact
sums (math.fsum).  It does not look at the kernel or at icp_flow_amd.  Shared by tests/test_buckets.py and
tests/test_gpu_buckets*.py.  Not a test module."""
import json
import math
import os

import numpy as np

import seqeval_restatement as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
EDGES = np.linspace(0.0, 2.0, 51)[1:]                 # 50 interior edges, metres per frame: 51 buckets, lower edge inclusive
CLASS_LO, ROWS = -1, 33
# the challenge's classes by name; a row's name: "UNLABELLED" (file value -1), the taxonomy by position (tests/golden/
# g16_argo_classes.json: file value = position, row = file value + 1), "OTHER" (everything else)
GROUP_NAMES = {
    "BACKGROUND": ["UNLABELLED", "BACKGROUND", "BOLLARD", "CONSTRUCTION_BARREL", "CONSTRUCTION_CONE", "MOBILE_PEDESTRIAN_CROSSING_SIGN", "SIGN",
                   "STOP_SIGN"],
    "CAR": ["REGULAR_VEHICLE"],
    "OTHER_VEHICLES": ["ARTICULATED_BUS", "BOX_TRUCK", "BUS", "LARGE_VEHICLE", "MESSAGE_BOARD_TRAILER", "RAILED_VEHICLE", "SCHOOL_BUS",
                       "TRAFFIC_LIGHT_TRAILER", "TRUCK", "TRUCK_CAB", "VEHICULAR_TRAILER"],
    "PEDESTRIAN": ["OFFICIAL_SIGNALER", "PEDESTRIAN", "STROLLER", "WHEELCHAIR"],
    "WHEELED_VRU": ["BICYCLE", "BICYCLIST", "MOTORCYCLE", "MOTORCYCLIST", "WHEELED_DEVICE", "WHEELED_RIDER"]}
UNGROUPED = ["ANIMAL", "DOG", "OTHER"]


def row_names():
    with open(os.path.join(REPO, "tests", "golden", "g16_argo_classes.json")) as f:
        return ["UNLABELLED"] + list(json.load(f)["names_by_position"]) + ["OTHER"]


def groups():
    """-> {class: sorted rows}"""
    names = row_names()
    return {g: sorted(names.index(n) for n in members) for g, members in GROUP_NAMES.items()}


def row_speed(gt):
    gt = np.asarray(gt, np.float64)
    x, y, z = gt[:, 0], gt[:, 1], gt[:, 2]
    return np.sqrt((x * x + y * y) + z * z)


class Cells:
    """counts int64 [G,S]; e and speed: per cell the list of the rows' values in row order; kept0, outside"""

    def __init__(self, G, S):
        self.counts = np.zeros((G, S), np.int64)
        self.e = [[[] for _ in range(S)] for _ in range(G)]
        self.speed = [[[] for _ in range(S)] for _ in range(G)]
        self.kept0 = self.outside = 0

    def lists(self, which):
        return self.e if which == "e" else self.speed

    def sums(self, which="e"):
        """math.fsum per cell -> float64 [G,S]"""
        return np.array([[math.fsum(c) for c in row] for row in self.lists(which)])

    def bounds(self, which="e"):
        """(n - 1) 2^-53 sum |x| per cell: what any order of the n - 1 additions of a cell's n values stays within of the exact
        sum, to first order (tests/class_restatement.py: Cells.bounds)"""
        return np.array([[max(len(c) - 1, 0) * U * math.fsum(abs(x) for x in c) for c in row] for row in self.lists(which)])

    def sequential(self, which="e"):
        out = np.zeros(self.counts.shape)
        for g, row in enumerate(self.lists(which)):
            for s, c in enumerate(row):
                acc = 0.0
                for x in c:
                    acc += x
                out[g, s] = acc
        return out

    def extend(self, other):
        """another sample's rows behind this one's -> self"""
        assert other.counts.shape == self.counts.shape
        self.counts += other.counts
        self.kept0 += other.kept0
        self.outside += other.outside
        for mine, theirs in ((self.e, other.e), (self.speed, other.speed)):
            for g, row in enumerate(theirs):
                for s, c in enumerate(row):
                    mine[g][s].extend(c)
        return self


def table(args, data, pred, classes, edges=EDGES, class_lo=CLASS_LO, G=ROWS, keep=None):
    """-> Cells.  data: raw_points, time_indice, scene_flow (numpy); args: num_frames and calculate_metrics' crop (`keep`: a row
    mask of the caller's instead).  A row counts when it passes the crop and its time index is in [1, F); its class row is
    value - class_lo for an integer value of [class_lo, class_lo + G - 2], else G - 1; its bucket the number of edges <= |gt|,
    0 for a NaN."""
    F = int(args.num_frames)
    edges = np.asarray(edges, np.float64).reshape(-1)
    raw, t = np.asarray(data["raw_points"]), np.asarray(data["time_indice"])
    keep = sr.keep_mask(args, raw) if keep is None else np.asarray(keep, bool)
    with np.errstate(all="ignore"):
        e, _ = sr.errors(data["scene_flow"], pred)
        speed = row_speed(data["scene_flow"])
        bucket = np.where(np.isnan(speed), 0, np.searchsorted(edges, speed, side="right")).astype(np.int64)
        cls = np.asarray(classes, np.float64)
    out = Cells(G, len(edges) + 1)
    out.outside = int(((t < 0) | (t >= F)).sum())
    out.kept0 = int((keep & (t == 0)).sum())
    for i in np.flatnonzero(keep & (t >= 1) & (t < F)).tolist():
        v = float(cls[i])
        g = int(v - class_lo) if math.isfinite(v) and v == math.floor(v) and class_lo <= v <= class_lo + G - 2 else G - 1
        s = int(bucket[i])
        out.counts[g, s] += 1
        out.e[g][s].append(float(e[i]))
        out.speed[g][s].append(float(speed[i]))
    return out


def metric(cells, by_class=None):
    """The bucket-normalised EPE from exact sums.  Per class (the groups, then OTHER = the rows in none): static = sum e / n of
    bucket 0 (NaN when empty); dynamic = the mean over the non-empty buckets b >= 1 of sum e_b / sum |gt|_b (NaN when there is
    none); n_static, n_dynamic, buckets_used.  mean_static / mean_dynamic: over the groups' classes, NaN skipped."""
    by_class = groups() if by_class is None else by_class
    G, S = cells.counts.shape
    used = sorted(r for rows in by_class.values() for r in rows)
    assert len(set(used)) == len(used)
    parts = dict(by_class, OTHER=[r for r in range(G) if r not in used])
    out = {}
    for name, rows in parts.items():
        e = [[x for r in rows for x in cells.e[r][b]] for b in range(S)]
        sp = [[x for r in rows for x in cells.speed[r][b]] for b in range(S)]
        static = math.fsum(e[0]) / len(e[0]) if e[0] else float("nan")
        with np.errstate(all="ignore"):
            ratios = [float(np.float64(math.fsum(e[b])) / np.float64(math.fsum(sp[b]))) for b in range(1, S) if e[b]]
        dynamic = math.fsum(ratios) / len(ratios) if ratios else float("nan")
        out[name] = dict(static=static, dynamic=dynamic, n_static=len(e[0]), n_dynamic=sum(len(c) for c in e[1:]), buckets_used=len(ratios))
    for key in ("static", "dynamic"):
        vals = [out[name][key] for name in by_class if not math.isnan(out[name][key])]
        out["mean_" + key] = math.fsum(vals) / len(vals) if vals else float("nan")
    return out


def metric_tolerance(n):
    """Relative distance allowed between a value of the metric computed from sums in ANY fixed order and `metric`'s: numerator
    and denominator are sums of at most n non-negative values, each within (n - 1) 2^-53 (relative, first order) of the exact
    sum whatever the tree; one division, the mean over at most 50 ratios (49 additions and a division) and the mean over five
    classes add fewer than 64 roundings."""
    return 2.0 * (n + 64) * U

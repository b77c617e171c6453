"""A plain numpy restatement of icpflow_seq_argo_sample (include/icpflow_hip.h), written from its description there, and the
g15 fixtures' access helpers, shared by tests/test_argo.py and tests/test_gpu_argo.py.  Not a test module."""
from types import SimpleNamespace

import numpy as np

from conftest import load_golden

SYNTHETIC = ("g15_argo_f32_int", "g15_argo_f32_float", "g15_argo_f64")
DEMO = "g15_argo_demo"
SAMPLE_KEYS = ("raw_points", "time_indice", "sd_labels", "fb_labels", "scene_flow")
# the three settings the fixtures' meters were recorded under: main.py's default ranges, main.sh:38's, eval_ground
SETTINGS = {"default": dict(range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3, eval_ground=False),
            "argo": dict(range_x=10000.0, range_y=10000.0, range_z=-10000.0, ground_slack=0.0, eval_ground=False),
            "ground": dict(range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3, eval_ground=True)}


def row_norm(flow):
    """|row| in the array's own dtype: the squares, (x x + y y) + z z, the square root -- each rounded by itself"""
    x, y, z = flow[:, 0], flow[:, 1], flow[:, 2]
    out = np.sqrt((x * x + y * y) + z * z)
    assert out.dtype == flow.dtype
    return out


def sd_threshold(dtype):
    """0.5 * 0.1 as numpy compares it with a norm of `dtype`"""
    return np.asarray(0.5 * 0.1, dtype=np.float64).astype(dtype)


def index_list(valid):
    valid = np.asarray(valid)
    return np.flatnonzero(valid) if valid.dtype == bool else valid.astype(np.int64)


def sample(pc1, pc2, flow, classes1, valid1, valid2, background):
    """-> dict(raw_points float64 [m,3], time_indice, sd_labels, fb_labels int32 [m], scene_flow float64 [m,3]), m = m2 + m1;
    every index must lie inside its cloud"""
    v1, v2 = index_list(valid1), index_list(valid2)
    assert ((v1 >= 0) & (v1 < len(pc1))).all() and ((v2 >= 0) & (v2 < len(pc2))).all()
    m1, m2 = len(v1), len(v2)
    f = flow[v1]
    with np.errstate(all="ignore"):
        sd = row_norm(f) > sd_threshold(flow.dtype)
    c = np.asarray(classes1)[v1].astype(np.float64)
    fb = ~(c == -1.0)
    for b in background:
        fb &= ~(c == float(b))
    zeros = np.zeros(m2, np.int32)
    return dict(raw_points=np.concatenate([pc2[v2], pc1[v1]]).astype(np.float64).reshape(m2 + m1, 3),
                time_indice=np.concatenate([zeros, np.ones(m1, np.int32)]),
                sd_labels=np.concatenate([zeros, sd.astype(np.int32)]), fb_labels=np.concatenate([zeros, fb.astype(np.int32)]),
                scene_flow=np.concatenate([np.zeros((m2, 3)), f.astype(np.float64)]).reshape(m2 + m1, 3))


def straddling_rows(dtype, seed=5, n=400_000):
    """Rows of `dtype` a few ulps around |row| = 0.05 for which (x x + y y) + z z and x x + (y y + z z) round differently AND
    fall on different sides of the threshold: the label tells the two association orders apart.  -> [k,3]"""
    rng = np.random.default_rng(seed)
    thr = sd_threshold(dtype)
    v = rng.normal(size=(n, 3))
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    v = (v * float(thr) * (1.0 + rng.uniform(-4, 4, size=(n, 1)) * np.finfo(dtype).eps)).astype(dtype)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    left, right = np.sqrt((x * x + y * y) + z * z), np.sqrt(x * x + (y * y + z * z))
    return v[(left > thr) != (right > thr)]


def load(name):
    return load_golden(name)


def file_arrays(name):
    """The file-form arrays of a fixture.  The demo sample's points, flow and prediction are not stored twice: they are
    g8_demo's valid rows, scattered here into 90 000-row arrays at seeded positions, NaN elsewhere.
    -> (dict of the file's keys, predicted flow float32 [m,3] with zeros for frame 0)"""
    g = load(name)
    if name != DEMO:
        return {k: g[k] for k in ("pc1", "pc2", "gt_flow_0_1", "pc1_classes", "pc2_classes", "ground1", "ground2",
                                  "pc1_flows_valid_idx", "pc2_flows_valid_idx")}, g["pred_flow"]
    g8 = load("g8_demo")
    n, rng = 90_000, np.random.default_rng(15)
    m1, m2 = len(g8["point_src"]), len(g8["point_dst"])
    v1, v2 = np.sort(rng.choice(n, m1, replace=False)), np.sort(rng.choice(n, m2, replace=False))
    pc1, pc2, flow = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
    cls = np.full(n, np.nan, np.float32)
    pc1[v1], pc2[v2], flow[v1], cls[v1] = g8["point_src"], g8["point_dst"], g8["gt_flow"], g["classes_valid"]
    pred = np.concatenate([np.zeros((m2, 3), np.float32), g8["flow"]])
    return dict(pc1=pc1, pc2=pc2, gt_flow_0_1=flow, pc1_classes=cls, pc1_flows_valid_idx=v1, pc2_flows_valid_idx=v2), pred


def recorded_sample(name):
    """What the reference's load_data_pca returned for the fixture's file (the demo sample's points and flow: g8_demo's)"""
    g = load(name)
    if name != DEMO:
        return {k: g["ref_" + k] for k in SAMPLE_KEYS}
    g8 = load("g8_demo")
    m2 = len(g8["point_dst"])
    return dict(raw_points=np.concatenate([g8["point_dst"], g8["point_src"]]),
                time_indice=np.concatenate([np.zeros(m2), np.ones(len(g8["point_src"]))]),
                sd_labels=g["ref_sd_labels"], fb_labels=g["ref_fb_labels"],
                scene_flow=np.concatenate([np.zeros((m2, 3)), g8["gt_flow"].astype(np.float64)]))


def setting_args(setting):
    return SimpleNamespace(num_frames=2, **SETTINGS[setting])


class Recorded:
    """One setting's recorded meters under the key names tests/seqeval_restatement.py reads (reference_table, check_meters)."""

    def __init__(self, g, setting):
        self.g, self.setting = g, setting

    def __getitem__(self, key):
        if key == "num_frames":
            return np.array(2)
        if key.startswith("eg0_"):
            return self.g[f"{self.setting}_{key[4:]}"]
        return self.g[key]

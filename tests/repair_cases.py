"""The inputs the tests of the track repair share (tests/test_tracks_repair.py on the CPU, tests/test_gpu_tracks_repair.py on the
GPU): hand-made observation tables for the plan, threshold tables for the select, and the end-to-end scene.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as tc                      # noqa: E402

F = np.float32
obs = tc.observation


# ------------------------------------------------------------------------------------------------------------------- the plan

def one_outlier(gaps=(1, 2, 3), bad=2, off=(0.0, 1.0, 0.0), v=(2.0, -1.0, 0.25), track=0, S=0.125):
    """a track seen once per gap at d = s v, the observation of gap `bad` moved by `off` (binary fractions: exact sums)"""
    rows = []
    for g in gaps:
        d = np.array(v) * (S * g) + (np.array(off) if g == bad else 0.0)
        rows.append(obs(track, g, S * g, d))
    return rows


def random_tables(count=300, seed=11):
    """seeded observation tables: ids -1, ids >= T, gaps outside [0, 63], +-0 displacements, several rows of a track in one gap"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        M, T = int(rng.integers(1, 40)), int(rng.integers(1, 6))
        v = rng.normal(0, 3, (T + 3, 3))
        rows = []
        for _ in range(M):
            t = int(rng.integers(-1, T + 2))
            g = int(rng.choice([-1, 0, 1, 2, 3, 5, 63, 64, 70]))
            s = 0.1 * max(g, 1)
            d = s * v[t + 1] + rng.normal(0, 0.1, 3) * (rng.random() < 0.4)
            if rng.random() < 0.2:
                d = np.array([0.0, -0.0, 0.0])
            rows.append(obs(t, g, s, d))
        yield np.array(rows), T


# ----------------------------------------------------------------------------------------------------------------- the select

IDENTITY = np.eye(4, dtype=F).reshape(16)


def translation(d):
    T = np.eye(4, dtype=F)
    T[:3, 3] = d
    return T.reshape(16)


def select_row(**over):
    """one pair of the select with every test passed by a wide margin: accepted"""
    row = dict(T_new=translation((1.0, 0.5, 0.0)), T_old=translation((2.0, 0.5, 0.0)), errors=(0.05, 0.06), ious=(0.9, 0.8), translations=(1.0, 0.5, 0.0),
               rotations=(3.0, 1.0, -2.0), errors_old=(0.1, 0.3), centre=(10.0, -4.0, 1.0), pred=(1.0, 0.5, 0.0))
    row.update(over)
    return row


def stack(rows):
    keys = ("T_new", "T_old", "errors", "ious", "translations", "rotations", "errors_old", "centre", "pred")
    return {k: np.array([r[k] for r in rows], np.float64 if k in ("centre", "pred") else F) for k in keys}


PARAMS = dict(translation_frame=1.25, thres_iou=0.25, rot_limit_deg=9.0, thres_error=0.25, max_residual=0.25)   # exact in float32


def threshold_rows():
    """-> (rows, the reason of each) under PARAMS: every reason reached, every threshold hit exactly and one float32 step beside"""
    up, down = (lambda x: np.nextafter(F(x), F(np.inf))), (lambda x: np.nextafter(F(x), F(-np.inf)))
    nan = F(np.nan)
    e, te = F(0.05), F(PARAMS["thres_error"])
    cases = [
        (select_row(), 0),
        # reason 1: the translation norm, min(iou) by the reference's rule, the two tested angles
        (select_row(translations=(1.25, 0.0, 0.0)), 0), (select_row(translations=(0.0, up(1.25), 0.0)), 1), (select_row(translations=(0.75, 0.0, 1.0)), 0),
        (select_row(translations=(nan, 0.0, 0.0)), 0),
        (select_row(ious=(0.25, 0.9)), 0), (select_row(ious=(down(0.25), 0.9)), 1), (select_row(ious=(0.9, down(0.25))), 1),
        (select_row(ious=(0.9, nan)), 0), (select_row(ious=(nan, 0.1)), 0), (select_row(ious=(0.1, nan)), 1),
        (select_row(rotations=(80.0, 9.0, -9.0)), 0), (select_row(rotations=(0.0, up(9.0), 0.0)), 1), (select_row(rotations=(0.0, 0.0, -up(9.0))), 1),
        (select_row(rotations=(0.0, nan, 50.0)), 0),
        # reason 2: e_new against thres_error in float32
        (select_row(errors=(down(te), 0.5), errors_old=(0.5, 0.5)), 0), (select_row(errors=(te, 0.5), errors_old=(0.5, 0.5)), 2),
        (select_row(errors=(up(te), 0.5), errors_old=(0.5, 0.5)), 2), (select_row(errors=(nan, 0.01)), 2), (select_row(errors=(0.01, nan)), 2),
        # reason 3: the new displacement exactly max_residual from the predicted one in xy (z does not count), and one step beyond
        (select_row(T_new=translation((1.0, 0.75, 9.0))), 0), (select_row(T_new=translation((1.0, up(0.75), 0.0))), 3),
        (select_row(T_new=translation((1.0, down(0.25), 0.0))), 3), (select_row(T_new=translation((nan, 0.5, 0.0))), 0),
        # reason 4: e_new against e_old; a NaN e_old is +inf
        (select_row(errors=(e, 0.06), errors_old=(e, 0.3)), 0), (select_row(errors=(e, 0.06), errors_old=(down(e), 0.3)), 4),
        (select_row(errors=(e, 0.06), errors_old=(up(e), 0.3)), 0), (select_row(errors=(e, 0.06), errors_old=(nan, 0.001)), 0),
        (select_row(errors=(e, 0.06), errors_old=(0.001, nan)), 0),
        # the order: the first failing test names the reason
        (select_row(ious=(0.0, 0.0), errors=(0.9, 0.9), T_new=translation((5.0, 0.0, 0.0))), 1),
        (select_row(errors=(0.9, 0.9), T_new=translation((5.0, 0.0, 0.0))), 2),
        (select_row(errors=(0.15, 0.16), T_new=translation((5.0, 0.0, 0.0))), 3),
    ]
    return [c for c, _ in cases], [r for _, r in cases]


# ------------------------------------------------------------------------------------------------------------------ the scene
# tests/track_cases.scene's construction with other boxes: box REPAIR_HONEST is long and leaves its line by 1 m ALONG its long
# side in the last frame -- slid back onto the line its long faces still lie on the destination's, so the slid pose passes the
# association's reject test and only its larger error speaks against it; box REPAIR_FAULTED moves at a constant velocity and is
# the one a test writes a fault into.
FRAMES, SWEEP_SECONDS, CLUSTER = tc.SCENE_FRAMES, tc.SCENE_SWEEP_SECONDS, dict(tc.SCENE_CLUSTER)
STEPS = np.array([[0.4, 0.0, 0.0], [-0.2, 0.3, 0.0], [0.0, -0.45, 0.0], [0.2, 0.1, 0.0], [0.0, 0.0, 0.0]])
CENTRES = np.array([[-15.0, -15.0, 0.8], [15.0, -15.0, 0.8], [-15.0, 15.0, 0.8], [15.0, 15.0, 0.8], [0.0, 0.0, 0.8]])
SIZES = np.array([[3.0, 1.6, 1.0], [3.0, 1.6, 1.0], [2.4, 1.4, 1.0], [10.0, 1.2, 0.4], [6.0, 0.0, 1.0]])    # the last: a wall
HONEST, HONEST_FRAME, HONEST_OFFSET = 3, 3, np.array([1.0, 0.0, 0.0])
FAULTED, FAULTED_FRAME, FAULT = 0, 2, np.array([1.0, 0.0, 0.0])       # 1 m along the box's long side, written into gap 2
WALL = 4


def displacement(k, j):
    """the true displacement of object k in gap j (frame j onto frame 0)"""
    return -(j * STEPS[k] + (HONEST_OFFSET if (k == HONEST and j == HONEST_FRAME) else 0.0))


def scene(seed=7, noise=0.005):
    """-> dict(arrays = load_sequence's keys, object [m] = the object of every row, -1 for noise), as tests/track_cases.scene"""
    rng = np.random.default_rng(seed)
    shapes = [tc._faces(rng, s) for s in SIZES]
    raw, tim, obj = [], [], []
    for j in range(FRAMES):
        for k, local in enumerate(shapes):
            raw.append(local + (CENTRES[k] - displacement(k, j)) + rng.normal(0.0, noise, local.shape))
            obj.append(np.full(len(local), k))
        raw.append(np.stack([np.linspace(-30, 30, 6), np.full(6, 30.0 + j), np.full(6, 0.5)], axis=1))
        obj.append(np.full(6, -1))
        tim.append(np.full(sum(len(s) for s in shapes) + 6, j))
    arrays = dict(raw_points=np.concatenate(raw).astype(F), time_indice=np.concatenate(tim).astype(np.int64), ego_motion=np.tile(np.eye(4), (FRAMES, 1, 1)))
    return dict(arrays=arrays, object=np.concatenate(obj))

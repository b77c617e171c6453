"""The inputs of tests/test_gpu_segment_residual.py that carry a condition of their own -- a condition the CPU suite asserts on
the restatement (tests/test_segment_residual.py), so that the GPU test cannot pass on a scene that does not exercise what it
names.  numpy only.  Not a test module."""
import numpy as np

SEGMENT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 777)
EDGES = (0.05, 0.1)


def label_values():
    """-> (labels float32 [n], segments expected): ground, noise, both zeros (one segment), two ordinary labels, a quiet NaN"""
    lab = np.array([-1e8, -1.0, 0.0, -0.0, 3.0, 3.0, 0.0, -1e8, np.nan, 7.0, -0.0, np.nan, -1.0], np.float32)
    return lab, 6


def lattice():
    """a cubic lattice of pitch 0.5 as the target (shuffled, some points twice), r = 0.5.  Rows 0 .. 149: BEFORE half a pitch
    from two lattice points (an exact tie, d = 0.25), AFTER -- by a flow of exactly one radius -- straight out of a face of the
    lattice, exactly r from the one target within reach: d2 == r2, a hit.  Rows 150 .. 299: the other way round.  Dyadic, so
    every operation is exact.  -> (before, after, flow, labels, target, radius)"""
    rng = np.random.default_rng(5)
    ax = np.arange(-4, 4) * 0.5
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    target = np.concatenate([grid, grid[rng.integers(0, len(grid), 100)]])[rng.permutation(len(grid) + 100)].astype(np.float32)
    on = grid[rng.integers(0, len(grid), 300)]
    face = on.copy()
    face[:, 1] = -2.0                                    # on the face y = -2 of the lattice
    tie = on.copy()
    tie[:, 0] += 0.25                                    # between two lattice points
    out = face.copy()
    out[:, 1] -= 0.5                                     # one radius outside the face
    before = np.concatenate([tie[:150], out[150:]])
    after = np.concatenate([face[:150], on[150:]])
    flow = np.zeros((300, 3))
    flow[:150, 1], flow[150:, 0] = -0.5, 0.25
    labels = rng.integers(0, 5, 300).astype(np.float32)
    return before.astype(np.float32), after.astype(np.float32), flow.astype(np.float32), labels, target, 0.5


def one_side_bad(n=600, m=700, seed=8):
    """rows that are bad on ONE side only: a flow of Inf (bad AFTER, good BEFORE), a pad row (1e8, 1e8, 1e8) in the source (bad
    on both sides: the flow is finite) and in the target.  -> (before, after, flow, labels, target, rows with the Inf flow, pad
    rows of the source, pad rows of the target)"""
    rng = np.random.default_rng(seed)
    target = rng.uniform(-4, 4, (m, 3)).astype(np.float32)
    before = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    flow = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    labels = rng.integers(0, 6, n).astype(np.float32)
    inf_rows, pad_src, pad_dst = np.arange(5, n, 97), np.arange(11, n, 131), np.arange(3, m, 101)
    flow[inf_rows, 1] = np.inf
    before[pad_src] = 1e8
    target[pad_dst] = 1e8
    return before, before.copy(), flow, labels, target, inf_rows, pad_src, pad_dst


def one_cell(n=400):
    """5 000 targets inside one cell of edge 2.02 (r = 2)"""
    rng = np.random.default_rng(12)
    target = rng.uniform(0.05, 1.95, (5000, 3)).astype(np.float32)
    before = rng.uniform(-2.5, 4.5, (n, 3)).astype(np.float32)
    flow = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    return before, before.copy(), flow, rng.integers(0, 3, n).astype(np.float32), target, 2.0


def rigid_pair(seed=41):
    """a synthetic.py frame pair whose destination is the rigidly moved source, dst = src + gt_flow rounded once
    -> dict(points_src, points_dst, labels_src, pose, gt_flow)"""
    from icp_flow_amd import synthetic
    d = synthetic.make_frame_pair(seed=seed, n_objects=6, n_min=60, n_max=400, n_background=600)
    dst = (d["points_src"].astype(np.float64) + d["gt_flow"].astype(np.float64)).astype(np.float32)
    return dict(points_src=d["points_src"], points_dst=dst, labels_src=d["labels_src"], pose=d["pose"], gt_flow=d["gt_flow"])


SABOTAGED = 2.0       # the label of the segment whose flow the verdict's scene spoils


def verdict(seed=41, sabotage=True):
    """the rigid pair with the ground-truth flow as the prediction; sabotage: (1, 0, 0) m added to the flow of segment SABOTAGED
    -> (before, after, flow, labels, target)"""
    d = rigid_pair(seed)
    flow = d["gt_flow"].copy()
    if sabotage:
        flow[d["labels_src"] == SABOTAGED] += np.array([1.0, 0.0, 0.0], np.float32)
    return d["points_src"], d["points_src"], flow, d["labels_src"], d["points_dst"]

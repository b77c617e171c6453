"""The skewed sequence of the deskewing tests (seeded; built in the test, nothing stored): a static world seen by a spinning
sensor on a constant twist, every point sampled at the pose of its own stamp."""
import numpy as np

import ego_deskew_restatement as dk
import ego_motion_scenes as scenes

# the sensor's motion per frame: 1.8 m forward, 0.1 m sideways, 4 degrees of yaw (18 m/s and 40 deg/s at 10 Hz: a fast turn)
TWIST = dk.se3_log(scenes.rigid(1.8, 0.1, 4.0))


def skewed_sequence(num_frames=6, n_points=4000, seed=0, twist=TWIST, noise=0.01, snapshots=2):
    """-> (frames, stamps, truth): float32 [n,3] in the sensor's coordinates, float32 [n] in [0, 1], float64 [F,4,4].
    The world is one fixed set of points (every frame sees all of them, with 1 cm of noise, in an order of its own), so a
    pose error is the skew's and not the sampling's.  The pose of frame j holds at stamp 0.5: truth[j] = exp(j twist).  A
    point's stamp is its azimuth's share of the turn (seen from truth[j]), and the point is seen from
    truth[j] exp((stamp - 0.5) twist): the sweep is smeared by the sensor's own motion, the more the farther the stamp is
    from the middle.

    The first `snapshots` frames are taken at once (every stamp 0.5).  No estimator can deskew them -- there is no motion
    estimate before two poses exist -- and a smeared frame 0 makes "frame j -> frame 0" ambiguous: with snapshots=0 the map
    starts from two smeared sweeps, which sit at a constant offset (measured with the restatement: 0.0137 rad) from every
    deskewed frame after them, and that offset, not the drift, is what a comparison with truth then shows."""
    rng = np.random.default_rng(8_300 + seed)

    def sample(n):
        k = n // 5
        ground = np.stack([rng.uniform(-30, 30, 2 * k), rng.uniform(-30, 30, 2 * k), rng.normal(-1.7, 0.02, 2 * k)], axis=1)
        side = np.where(rng.random(k) < 0.5, -9.0, 11.0)
        walls = np.stack([rng.uniform(-30, 30, k), side + 0.3 * np.sin(np.arange(k)), rng.uniform(-1.7, 4.0, k)], axis=1)
        cross = np.stack([np.where(rng.random(k) < 0.5, -19.0, 23.0), rng.uniform(-30, 30, k), rng.uniform(-1.7, 5.0, k)], axis=1)
        centres = np.array([[x, y] for x in range(-25, 30, 10) for y in (-6.0, 7.0)])
        c = centres[rng.integers(0, len(centres), n - 4 * k)]
        ang = rng.uniform(0, 2 * np.pi, len(c))
        poles = np.stack([c[:, 0] + 0.15 * np.cos(ang), c[:, 1] + 0.15 * np.sin(ang), rng.uniform(-1.7, 3.0, len(c))], axis=1)
        return np.concatenate([ground, walls, cross, poles])

    fixed = sample(n_points)                       # the world is one fixed set of points: every frame sees all of them
    frames, stamps, truth = [], [], []
    for j in range(num_frames):
        P = dk.se3_exp(j * np.asarray(twist))
        world = (fixed + rng.normal(0.0, noise, size=(n_points, 3)))[rng.permutation(n_points)]
        nominal = (world - P[0:3, 3]) @ P[0:3, 0:3]
        s = ((np.arctan2(nominal[:, 1], nominal[:, 0]) + np.pi) / (2.0 * np.pi)).astype(np.float32)
        if j < snapshots:
            s[:] = 0.5
        pts = dk.deskew(nominal, s, -np.asarray(twist))          # exp(-(stamp - 0.5) twist) inv(truth[j]) world
        frames.append(pts)
        stamps.append(s)
        truth.append(P)
    return frames, stamps, np.stack(truth)


_runs = {}


def skewed_runs():
    """(frames, stamps, truth, the restatement's run without deskewing, with) -- once per session"""
    if not _runs:
        frames, stamps, truth = skewed_sequence()
        odos = []
        for on in (False, True):
            odo = dk.StampedOdometry(deskew=on)
            for f, s in zip(frames, stamps):
                odo.register_frame(f, s, keep_map=False)
            odos.append(odo)
        _runs["x"] = (frames, stamps, truth, odos[0], odos[1])
    return _runs["x"]


# ---- the inputs of the kernel test (tests/test_gpu_ego_deskew.py) and of the CPU test that derives its bound ------------------
KERNEL_SIZES = (1, 63, 64, 65, 4097)           # one point, around a wave, more than one block with a ragged last one
SPECIAL_STAMPS = (0.0, 0.5, 1.0, -0.25, 1.5, np.nan)


def _twist(rho, axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    return np.concatenate([np.asarray(rho, dtype=np.float64), angle * axis / np.linalg.norm(axis)])


# name -> (rho, omega).  With stamps in [-0.25, 1.5], d = stamp - 0.5 is in [-0.75, 1]: an angle of 2^-12 puts |d| = 0.5 (the
# stamps 0 and 1) on the library's switch 2^-13 and the points on both sides of it, 2e-5 does the same for the restatement's.
KERNEL_TWISTS = dict(
    zero=np.zeros(6),
    translation=_twist([1.5, -0.2, 0.05], [0, 0, 1], 0.0),
    tiny=_twist([1.5, -0.2, 0.05], [0.2, -0.1, 1.0], 2e-9),             # theta d = 1e-9 at the ends of the sweep
    switch_library=_twist([1.5, -0.2, 0.05], [0.2, -0.1, 1.0], 2.0 ** -12),
    switch_restatement=_twist([1.5, -0.2, 0.05], [0.2, -0.1, 1.0], 2e-5),
    turn=_twist([1.5, -0.2, 0.05], [0.2, -0.1, 1.0], 0.3),
    half_turn_nearly=_twist([1.5, -0.2, 0.05], [0.2, -0.1, 1.0], np.pi - 1e-3))


def kernel_case(name, n):
    """-> (points float32 [n,3] up to 100 m, stamps float32 [n], poses float64 [2,4,4] = (identity, exp(twist)))"""
    rng = np.random.default_rng(8_400 + 31 * n + sorted(KERNEL_TWISTS).index(name))
    points = rng.uniform(-100.0, 100.0, size=(n, 3)).astype(np.float32)
    stamps = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if n >= len(SPECIAL_STAMPS):
        stamps[np.linspace(0, n - 1, len(SPECIAL_STAMPS)).astype(int)] = SPECIAL_STAMPS
    else:
        stamps[:] = SPECIAL_STAMPS[2]
    return points, stamps, np.stack([np.eye(4), dk.se3_exp(KERNEL_TWISTS[name])])


def ulps_apart(a, b):
    """float32 arrays -> how many representable values lie between a and b, per element (both finite)"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))

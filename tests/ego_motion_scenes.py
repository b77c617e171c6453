"""Scenes with a known ego motion for the ego-motion tests (seeded; built in the test, nothing stored)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_demo.npz")


def rigid(forward=0.0, sideways=0.0, yaw_deg=0.0, up=0.0):
    a = np.deg2rad(yaw_deg)
    P = np.eye(4)
    P[0:3, 0:3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    P[0:3, 3] = [forward, sideways, up]
    return P


def into_frame(points, pose):
    """world (= frame 0) points as the sensor at `pose` sees them: inv(pose) p, fp64 -> float32"""
    p = np.asarray(points, dtype=np.float64)
    R, t = pose[0:3, 0:3], pose[0:3, 3]
    return ((p - t) @ R).astype(np.float32)


def demo_clouds():
    with np.load(GOLDEN) as z:
        return np.ascontiguousarray(z["point_dst"][:, 0:3], dtype=np.float32), np.ascontiguousarray(z["point_src"][:, 0:3], dtype=np.float32)


def real_pair():
    """The real ego-compensated LiDAR frame pair: frame 0 = point_dst, frame 1 = point_src seen from P.  The true
    poses[1] is P up to the data set's own pose error and the moving objects.  -> (frames, poses)"""
    dst, src = demo_clouds()
    P = rigid(1.2, 0.3, 1.5)
    return [dst, into_frame(src, P)], np.stack([np.eye(4), P])


def exact_path(num_frames=5, seed=0, step=rigid(1.2, 0.0, 0.6), noise=0.01, keep=0.9):
    """Frames 1.. made from point_dst itself (a random 90 % subset, 1 cm noise) along a constant-velocity path: truth
    is exact, the sensor moves more than 2.5 m (the adaptive threshold takes over), the constant-velocity guess is
    used from frame 2 on.  -> (frames, poses)"""
    dst, _ = demo_clouds()
    rng = np.random.default_rng(8_100 + seed)
    frames, poses, P = [dst], [np.eye(4)], np.eye(4)
    for _ in range(1, num_frames):
        P = P @ step
        sub = np.sort(rng.choice(len(dst), int(keep * len(dst)), replace=False))
        world = dst[sub].astype(np.float64) + rng.normal(0.0, noise, size=(len(sub), 3))
        frames.append(into_frame(world, P))
        poses.append(P.copy())
    return frames, np.stack(poses)


def synthetic_static(num_frames=4, seed=0, n_points=30000, step=rigid(0.9, 0.05, -0.8), noise=0.01):
    """A dense static scene of the tests' own (synthetic.make_sequence's 1500 ground points are a flat sheet, about one
    per 1.5 m voxel, and most of its objects move: no odometry recovers truth from it): a ground sheet, walls along a
    street and across it, and poles, sampled afresh for every frame.  -> (frames, poses)"""
    rng = np.random.default_rng(8_200 + seed)

    def sample(n):
        k = n // 5
        ground = np.stack([rng.uniform(-40, 40, 2 * k), rng.uniform(-40, 40, 2 * k), rng.normal(-1.7, 0.02, 2 * k)], axis=1)
        side = np.where(rng.random(k) < 0.5, -9.0, 11.0)
        walls = np.stack([rng.uniform(-40, 40, k), side + 0.3 * np.sin(np.arange(k)), rng.uniform(-1.7, 4.0, k)], axis=1)
        cross = np.stack([np.where(rng.random(k) < 0.5, -27.0, 31.0), rng.uniform(-40, 40, k), rng.uniform(-1.7, 5.0, k)], axis=1)
        centres = np.array([[x, y] for x in range(-35, 40, 10) for y in (-6.0, 7.0)])
        c = centres[rng.integers(0, len(centres), n - 4 * k)]
        ang = rng.uniform(0, 2 * np.pi, len(c))
        poles = np.stack([c[:, 0] + 0.15 * np.cos(ang), c[:, 1] + 0.15 * np.sin(ang), rng.uniform(-1.7, 3.0, len(c))], axis=1)
        return np.concatenate([ground, walls, cross, poles])

    frames, poses, P = [], [], np.eye(4)
    for j in range(num_frames):
        world = sample(n_points) + rng.normal(0.0, noise, size=(n_points, 3))
        frames.append(into_frame(world[rng.permutation(n_points)], P))
        poses.append(P.copy())
        P = P @ step
    return frames, np.stack(poses)


def cap_expression(pose, truth):
    """|dt| + 50 m * dtheta: what a static point at 50 m is displaced by under the pose error"""
    from ego_motion_restatement import pose_error
    dt, dth = pose_error(pose, truth)
    return dt + 50.0 * dth

"""The yardstick of the deskewing tests: the motion compensation and the fixed threshold of include/icpflow_hip.h ("8(f), second
configuration") restated in plain fp64 numpy, on top of tests/ego_motion_restatement.py (imported, not copied).  Test code,
not product code: the formulas are the contract's as written -- theta = |d omega|, K = [d omega]_x, the three coefficients
A, B, C per point -- where the HIP kernel scales a unit axis by a signed angle and takes one sincos of the half angle; the
log solves V rho = t with numpy where the library has the closed form of V^-1.

    xi = se3_log(T)                         # (rho, omega) float64 [6]
    T = se3_exp(xi)                         # float64 [4,4]
    out = deskew(points, stamps, xi)        # float32 [n,3]: every point moved by exp((stamp - mid) xi), rounded once
    odo = StampedOdometry(deskew=True)      # Odometry + per-point stamps + fixed_threshold
    pose = odo.register_frame(points, stamps)
"""
import numpy as np

import ego_motion_restatement as rest

SERIES_BELOW = 1e-5     # the restatement's own switch to the series of A, B, C (the library's is 2^-13, stated in the header)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def coefficients(theta, sin=np.sin):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 for an array of angles; series below SERIES_BELOW.
    1 - cos t is taken as 2 sin^2(t / 2): the difference itself is good to 1e-16 only, which B K rho turns into
    1e-16 |rho| / t metres (measured against the power series: 3e-14 at t = 2.4e-4)."""
    theta = np.asarray(theta, dtype=np.float64)
    t2 = theta * theta
    with np.errstate(all="ignore"):
        s, h = sin(theta), sin(0.5 * theta)
        small = theta < SERIES_BELOW
        A = np.where(small, 1.0 - t2 / 6.0, s / theta)
        B = np.where(small, 0.5 - t2 / 24.0, 2.0 * h * h / t2)
        C = np.where(small, 1.0 / 6.0 - t2 / 120.0, (theta - s) / (t2 * theta))
    return A, B, C


def se3_exp(xi):
    xi = np.asarray(xi, dtype=np.float64)
    rho, omega = xi[0:3], xi[3:6]
    A, B, C = (float(v) for v in coefficients(np.linalg.norm(omega)))
    K = hat(omega)
    T = np.eye(4)
    T[0:3, 0:3] = np.eye(3) + A * K + B * (K @ K)
    T[0:3, 3] = (np.eye(3) + B * K + C * (K @ K)) @ rho
    return T


def se3_log(T):
    """(rho, omega) of a rigid motion with a rotation below a half turn"""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[0:3, 0:3], T[0:3, 3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(v))
    theta = float(np.arctan2(s, 0.5 * (np.trace(R) - 1.0)))
    omega = v * (theta / s) if s > 0.0 else v
    _, B, C = (float(x) for x in coefficients(theta))
    K = hat(omega)
    rho = np.linalg.solve(np.eye(3) + B * K + C * (K @ K), t)
    return np.concatenate([rho, omega])


def deskew(points, stamps, xi, mid_stamp=0.5, sin=np.sin):
    """p' = R p + V (d rho) with exp(d xi) = (R | V d rho), d = stamp - mid_stamp, per point in fp64 -> float32 [n,3].
    `sin`: the function the coefficients are taken from (the CPU test perturbs it by a few ulps)."""
    p = np.asarray(points, dtype=np.float64)[:, 0:3]
    xi = np.asarray(xi, dtype=np.float64)
    d = np.asarray(stamps, dtype=np.float32).astype(np.float64) - float(mid_stamp)
    with np.errstate(all="ignore"):
        om, rh = d[:, None] * xi[None, 3:6], d[:, None] * xi[None, 0:3]
        A, B, C = (v[:, None] for v in coefficients(np.linalg.norm(om, axis=1), sin))
        kp = np.cross(om, p)
        kr = np.cross(om, rh)
        out = (p + A * kp + B * np.cross(om, kp)) + (rh + B * kr + C * np.cross(om, kr))
        return out.astype(np.float32)


class StampedOdometry(rest.Odometry):
    """rest.Odometry with the second configuration: step 0 before every frame that comes with stamps, and sigma fixed"""

    def __init__(self, deskew=False, mid_stamp=0.5, fixed_threshold=0.0, **over):
        super().__init__(**over)
        self.deskew, self.mid_stamp, self.fixed_threshold = bool(deskew), float(mid_stamp), float(fixed_threshold)

    def threshold(self):
        return self.fixed_threshold if self.fixed_threshold > 0.0 else super().threshold()

    def correct(self, points, stamps):
        points = np.ascontiguousarray(points, dtype=np.float32)[:, 0:3]
        if not self.deskew or stamps is None or len(self.poses) < 2:
            return points
        return deskew(points, stamps, se3_log(rest.rigid_inverse(self.poses[-2]) @ self.poses[-1]), self.mid_stamp)

    def register_frame(self, points, stamps=None, keep_map=True):
        corrected = self.correct(points, stamps)
        with np.errstate(invalid="ignore"):          # (a row that is not finite fails the crop's comparisons)
            pose = super().register_frame(corrected, keep_map)
        self.records[-1]["corrected"] = corrected
        return pose

"""A plain NumPy restatement of match_eval (icpflow_match_eval, row a-12; no GPU, no torch), written from the comments of
csrc/nn.hip, scan.hpp, common.hpp and pose.hip (eval_epilogue_kernel) and from utils_match.py:159-213, not from the kernels' paths:

  * a cloud's length is its number of rows with w > 0, a prefix (the pad_segment layout); only those rows are queries or targets;
  * the moved cloud is pcd1 under the pose, per coordinate fmaf(z, m2, fmaf(y, m1, fl(x * m0))) + t (`moved`);
  * forward: every moved row's nearest row of pcd2; backward: every row of pcd2's nearest MOVED row.  The squared distance is
    fmaf(dz, dz, fmaf(dy, dy, fl(dx * dx))) of the float32 differences query - target, the minimum over the targets is taken of
    those float32 numbers, the distance is its float32 square root (`min_d2`, `pair`);
  * an inlier is a row with d < float32(thres_dist), strictly;
  * the sums over the rows -- distances, inlier flags, moved and original coordinates -- are exact here (math.fsum); the library
    forms them in float64 in an order of its own, which is what `sum_bounds` allows for;
  * the epilogue is eval_epilogue_kernel's, operation by operation in float32 (`epilogue`).

Every float32 operation is a NumPy float32 operation on float32 operands; the fused one is sort_restatement.fma32.

`min_d2(select=True)` evaluates the float32 chain only where it can matter: the float64 value of dx^2 + dy^2 + dz^2 (from the same
float32 differences) is within 3 * 2^-24 relative of the chain's result -- one rounding per operation --, so the chain's minimum is
attained among the targets whose float64 value lies within 1e-6 relative of the float64 minimum.  tests/test_match_eval_restatement.py
shows that this equals the plain form.
"""
import math

import numpy as np

import sort_restatement as sr

F = np.float32
INF = F(np.inf)
PI_F = F(3.14159265358979323846)
fma32 = sr.fma32


def length(cloud):
    return int((np.asarray(cloud)[:, 3] > 0).sum())


def moved(points, M):
    """rows [n, 3] float32 under the pose M [4, 4] float32, as affine_apply forms them"""
    p, M = np.asarray(points, F).reshape(-1, 3), np.asarray(M, F)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = fma32(p[:, 2], M[r, 2], fma32(p[:, 1], M[r, 1], p[:, 0] * M[r, 0])) + M[r, 3]
    return out


def sqdist(q, t):
    """the float32 chain on broadcastable rows [.., 3]"""
    dx, dy, dz = q[..., 0] - t[..., 0], q[..., 1] - t[..., 1], q[..., 2] - t[..., 2]
    return fma32(dz, dz, fma32(dy, dy, dx * dx))


def min_d2(Q, T, select=True, rows=256):
    """the smallest float32 squared distance of every row of Q [nq, 3] to the rows of T [nt, 3]; +inf without targets"""
    Q, T = np.asarray(Q, F).reshape(-1, 3), np.asarray(T, F).reshape(-1, 3)
    out = np.full(len(Q), INF, F)
    if len(T) == 0:
        return out
    for i in range(0, len(Q), rows):
        q = Q[i:i + rows]
        dx, dy, dz = (q[:, None, k] - T[None, :, k] for k in range(3))
        if not select:
            out[i:i + rows] = fma32(dz, dz, fma32(dy, dy, dx * dx)).min(axis=1)
            continue
        a, b, c = dx.astype(np.float64), dy.astype(np.float64), dz.astype(np.float64)
        e = a * a + b * b + c * c
        r, k = np.nonzero(e <= e.min(axis=1)[:, None] * (1.0 + 1e-6))
        x, y, z = dx[r, k], dy[r, k], dz[r, k]
        np.minimum.at(out[i:i + rows], r, fma32(z, z, fma32(y, y, x * x)))
    return out


def pair(p1, p2, M, thres, select=True):
    """One pair of clouds [N, 4] under the pose M -> dict: n1, n2, d (the two directions' float32 distances per valid row),
    inl (their inlier flags), S (the exact sums of d, as float), I (inlier counts), Sm / So (sums of the moved / original
    coordinates of pcd1), A (sums of their magnitudes), mv (the moved rows)."""
    p1, p2 = np.asarray(p1, F), np.asarray(p2, F)
    n1, n2 = length(p1), length(p2)
    a, c = p1[:n1, :3], p2[:n2, :3]
    mv = moved(a, M)
    th = F(thres)
    with np.errstate(all="ignore"):
        d = [np.sqrt(min_d2(mv, c, select)), np.sqrt(min_d2(c, mv, select))]
    inl = [x < th for x in d]
    col = lambda v: [math.fsum(v[:, k].astype(np.float64)) for k in range(3)]     # noqa: E731
    return dict(n1=n1, n2=n2, d=d, inl=inl, S=[math.fsum(x.astype(np.float64)) for x in d], I=[int(x.sum()) for x in inl],
                Sm=col(mv), So=col(a), Am=col(np.abs(mv)), Ao=col(np.abs(a)), mv=mv)


def rotations32(M):
    """pytorch3d's matrix_to_euler_angles(.., 'ZYX') * 180. / pi on float32, in the kernel's order of operations"""
    M = np.asarray(M, F)
    with np.errstate(all="ignore"):
        ang = [np.arctan2(M[1, 0], M[0, 0]), np.arcsin(-M[2, 0]), np.arctan2(M[2, 1], M[2, 2])]
        return np.array([(F(v) * F(180.0)) / PI_F for v in ang], F)


def rotations64(M):
    """the same angles of the same float32 entries, evaluated in float64"""
    M = np.asarray(M, F).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.array([np.arctan2(M[1, 0], M[0, 0]), np.arcsin(-M[2, 0]), np.arctan2(M[2, 1], M[2, 2])]) * 180.0 / np.pi


def epilogue(r, M):
    """eval_epilogue_kernel on the sums of `pair` -> dict of float32 arrays: errors, inliers, ratios, ious [2]; translations,
    rotations [3]"""
    with np.errstate(all="ignore"):
        n1, n2, n12 = F(r["n1"]), F(r["n2"]), F(r["n1"] + r["n2"])
        s1, s2, in1, in2 = F(r["S"][0]), F(r["S"][1]), F(r["I"][0]), F(r["I"][1])
        tr = [F(r["Sm"][k]) / n1 - F(r["So"][k]) / n1 for k in range(3)]
        return dict(errors=np.array([s1 / n1, s2 / n2], F), inliers=np.array([in1, in2], F), ratios=np.array([in1 / n1, in2 / n2], F),
                    ious=np.array([in1 / (n12 - in2), in2 / (n12 - in1)], F), translations=np.array(tr, F), rotations=rotations32(M))


def batch(P1, P2, T, thres, select=True):
    """-> (per-pair `pair` records, dict of [B, 2] / [B, 3] float32 arrays as the call returns them)"""
    recs = [pair(a, c, M, thres, select) for a, c, M in zip(P1, P2, T)]
    eps = [epilogue(r, M) for r, M in zip(recs, T)]
    return recs, {k: np.stack([e[k] for e in eps]) for k in eps[0]}


def sum_bounds(S, A, n):
    """What float32(sum) / n can be when the sum of n float64 terms is formed in ANY order: every partial sum is at most A = sum |x|
    in magnitude, each of the n - 1 additions rounds once, so the computed sum is within (n - 1) 2^-53 A of the exact S.  Rounding
    to float32 and dividing by float32(n) are monotone.  -> (low, high) float32"""
    with np.errstate(all="ignore"):
        if not np.isfinite(S) or n <= 0:
            v = F(S) / F(n)
            return v, v
        delta = (n - 1) * 2.0 ** -53 * A
        return F(S - delta) / F(n), F(S + delta) / F(n)


def translation_bounds(r):
    """the interval of every translation component: `sum_bounds` on either centroid, carried through the float32 subtraction"""
    lo, hi = [], []
    for k in range(3):
        ml, mh = sum_bounds(r["Sm"][k], r["Am"][k], r["n1"])
        ol, oh = sum_bounds(r["So"][k], r["Ao"][k], r["n1"])
        with np.errstate(all="ignore"):
            lo.append(ml - oh)
            hi.append(mh - ol)
    return np.array(lo, F), np.array(hi, F)

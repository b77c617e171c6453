"""The Kabsch solve of the ICP iteration (csrc/kabsch.hpp: Horn's closed form, its rank-1 fallback, the
allow_reflection mirror) against an fp64 SVD, on the degenerate inputs where closed forms go wrong:
planar, near-collinear, rank-1 and zero H, isotropic H, det H < 0 with nearly equal singular values,
half turns, magnitudes from 1e-10 to 1e6, and H / gsum built from small fp32 point sets the way the
ICP kernel builds them.  icpflow_selftest_kabsch runs the kernels' own solve, one wave per matrix.

Reference (utils_icp_pytorch3d.py:339-374, row convention y = x R): H = U S V^T, d = sign det(U V^T),
R* = U diag(1, 1, d) V^T, sigma* = s1 + s2 + d s3 = max over proper rotations of sum_ij R_ij H_ij
(allow_reflection: d = 1, the best orthogonal matrix).  The checks are on that objective, so that
they hold whichever maximiser is returned where it is not unique.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
EPS = np.finfo(np.float64).eps

# objective / scale-numerator bounds, relative to |H|_F
LOOSE = 1e-7          # every input
TIGHT = 1e-12         # where the top eigenvalue of N(H) is separated by >= 1e-3 |H|_F
R_TIGHT = 1e-10       # |R - R*| there
ORTHO = 1e-13
# det H < 0 with s1 ~ s2 ~ |s3| (N's eigenvalues 1 + e and a double 1 - e): the adjugate of the closed form
# cancels below e ~ 3.6e-5 and the rank-1 fallback answers a rank-3 H.  Its rotation is optimal on the
# double eigenvalue's subspace only, short of sigma* by up to ~2 e |H|; the scale numerator is
# the objective of that rotation, not |H|_F.  A correct eigenvector on that path is not in this change (every form
# of it tried so far changes the register allocation of all ICP kernels).  Above that, Newton's early exit leaves
# lambda ~1e-11 |H| off (the second root lies 2e below the top one), which only the scale sees.
# The scale numerator from Newton's root where the top eigenvalue of N is (nearly) double -- rank(H) <= 1, near-collinear
# points, det H < 0 with s2 ~ |s3| -- is good to ~sqrt(eps) only, the limit of a characteristic-polynomial method
# (measured: 3.3e-7 |H|); the rotation is not affected (LOOSE holds for the objective).  Only estimate_scale reads it.
LAM_LOOSE = 1e-6
DOUBLE_TOP = 1e-4
DOUBLE_TOP_LAM = 1e-9
DOUBLE_TOP_R = 1e-6   # the adjugate's eigenvector there is good to ~eps / e^2 relative


def rot(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[np.linalg.det(q) < 0, :, 0] *= -1.0
    return q


def axis_angle(axis, ang):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def from_sv(rng, S):
    """H = U diag(s) V^T for rows s of S (s3 may be negative: det H < 0)."""
    S = np.asarray(S, dtype=np.float64)
    U, V = rot(rng, len(S)), rot(rng, len(S))
    return np.einsum("bij,bj,bkj->bik", U, S, V)


def moments(X, Y):
    """H and gsum of an fp32 point pair as icp.hip forms them (weights 1): centred second moments / W."""
    X = X.astype(np.float32).astype(np.float64)
    Y = Y.astype(np.float32).astype(np.float64)
    W = float(len(X))
    mx, my = X.sum(0) / W, Y.sum(0) / W
    H = (X.T @ Y) / W - np.outer(mx, my)
    sxx = (X * X).sum() / W - mx @ mx
    syy = (Y * Y).sum() / W - my @ my
    return H, sxx + syy


def families():
    rng = np.random.default_rng(20261016)
    fam = {}
    n = 64
    fam["generic"] = (from_sv(rng, np.sort(rng.random((n, 3)) + 0.05, axis=1)[:, ::-1]), None)
    fam["planar"] = (from_sv(rng, np.c_[1 + rng.random(n), rng.random(n) * 0.9 + 0.05, np.zeros(n)]), None)
    small = 10.0 ** -rng.uniform(3, 12, n)
    fam["near_collinear"] = (from_sv(rng, np.c_[np.ones(n), small, small * rng.random(n)]), None)
    u, v = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    fam["rank1"] = (np.einsum("b,bi,bj->bij", 10.0 ** rng.uniform(-3, 3, n), u, v), None)
    fam["isotropic"] = (from_sv(rng, np.ones((n, 3)) * (1 + 1e-14 * rng.standard_normal((n, 3)))), None)
    g = np.r_[10.0 ** -np.linspace(2, 10, n - 8), np.zeros(8)]
    fam["reflect_s2_eq_s3"] = (from_sv(rng, np.c_[np.full(n, 2.0), np.ones(n), -(1 - g)]), None)
    e = 10.0 ** -np.linspace(2, 9, n)
    fam["reflect_double_top"] = (from_sv(rng, np.c_[np.ones(n), np.ones(n), -(1 - e)]), None)
    # half turns and near-half turns (q0 ~ 0): H = P Rh with P = U S U^T symmetric positive definite, so that R* = Rh
    Uh = rot(rng, n)
    P = np.einsum("bij,bj,bkj->bik", Uh, np.c_[3 + rng.random(n), 2 + rng.random(n), 1 + rng.random(n)], Uh)
    ax = rng.standard_normal((n, 3))
    ang = np.pi - np.r_[np.zeros(n // 2), 10.0 ** -rng.uniform(1, 12, n - n // 2)]
    Rh = np.stack([axis_angle(ax[i], ang[i]) for i in range(n)])
    fam["half_turn"] = (np.einsum("bij,bjk->bik", P, Rh), None)
    mags = 10.0 ** np.linspace(-10, 6, n)
    fam["magnitudes"] = (from_sv(rng, np.sort(rng.random((n, 3)) + 0.05, axis=1)[:, ::-1]) * mags[:, None, None], None)
    # H and gsum from fp32 point sets (2, 3, 4 points, exact planes and lines, Y = X R exactly)
    Hs, gs = [], []
    for i in range(n):
        k = (2, 3, 4, 6)[i % 4]
        X = rng.standard_normal((k, 3)).astype(np.float32)
        if i % 8 == 4:
            X[:, 2] = np.float32(0.5)                 # fp32-exact plane
        if i % 8 == 6:
            X = (np.arange(k, dtype=np.float32)[:, None] * np.float32([1, 2, -0.5])).astype(np.float32)   # exact line
        R0 = rot(rng, 1)[0] if i % 3 else np.eye(3)[[1, 0, 2]] * np.array([[1], [-1], [1]])   # exact 90 deg turns too
        if i % 5 == 2:
            R0 = np.diag([-1.0, -1.0, 1.0])                                    # an exact half turn
        Y = (X.astype(np.float64) @ R0).astype(np.float32)
        H, gsum = moments(X, Y)
        Hs.append(H)
        gs.append(gsum)
    fam["points_fp32"] = (np.stack(Hs), np.array(gs))
    return fam


def test_half_turn_family_is_made_of_half_turns():
    H = families()["half_turn"][0]
    U, _, Vt = np.linalg.svd(H)
    R = U @ Vt
    ang = np.arccos(np.clip((np.trace(R, axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert (np.pi - ang <= 0.1 + 1e-6).all() and (np.pi - ang < 1e-6).sum() >= len(H) // 2


def reference(H, mirror):
    U, S, Vt = np.linalg.svd(H)
    d = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
    if mirror:
        d = np.ones_like(d)
    E = np.ones((len(H), 3))
    E[:, 2] = d
    Rstar = np.einsum("bij,bj,bjk->bik", U, E, Vt)
    sig = S[:, 0] + S[:, 1] + d * S[:, 2]
    s3 = d * S[:, 2]
    lams = np.stack([S[:, 0] + S[:, 1] + s3, S[:, 0] - S[:, 1] - s3, -S[:, 0] + S[:, 1] - s3, -S[:, 0] - S[:, 1] + s3], 1)
    lams = -np.sort(-lams, axis=1)
    frob = np.linalg.norm(H.reshape(len(H), 9), axis=1)
    gap = (lams[:, 0] - lams[:, 1]) / np.where(frob > 0, frob, 1.0)
    if mirror:   # the best orthogonal matrix: flipping the third singular direction costs 2 s3
        gap = np.minimum(gap, 2 * S[:, 2] / np.where(frob > 0, frob, 1.0))
    return Rstar, sig, gap, frob


def solve(H, gsum, mode):
    n = len(H)
    dH = torch.from_numpy(np.ascontiguousarray(H.reshape(n, 9))).to(DEV)
    dg = torch.from_numpy(np.ascontiguousarray(gsum)).to(DEV)
    R = torch.empty((n, 9), dtype=torch.float64, device=DEV)
    lam = torch.empty(n, dtype=torch.float64, device=DEV)
    path = torch.empty(n, dtype=torch.int32, device=DEV)
    _lib.call("icpflow_selftest_kabsch", _lib.ptr(dH), _lib.ptr(dg), n, mode, _lib.ptr(R), _lib.ptr(lam), _lib.ptr(path),
              _lib.stream(DEV))
    torch.cuda.synchronize()
    return R.cpu().numpy().reshape(n, 3, 3), lam.cpu().numpy(), path.cpu().numpy()


def start(H, gsum):
    """icp.hip's Newton start where the family has no point sets behind it: an upper bound of 2 sigma*."""
    if gsum is not None:
        return gsum
    S = np.linalg.svd(H, compute_uv=False)
    return 2.0 * S.sum(1) * (1 + 1e-12)


def check(name, H, gsum, mode, report):
    mirror = mode == 1
    R, lam, path = solve(H, start(H, gsum), mode)
    Rstar, sig, gap, frob = reference(H, mirror)
    scale = np.where(frob > 0, frob, 1.0)
    I = np.eye(3)
    orth = np.abs(np.einsum("bji,bjk->bik", R, R) - I).max(axis=(1, 2))
    det = np.linalg.det(R)
    want_det = np.where(mirror & (np.linalg.det(H) < 0), -1.0, 1.0)
    obj = np.einsum("bij,bij->b", R, H)
    short = (sig - obj) / scale
    lerr = np.abs(lam - sig) / scale
    sep = gap >= 1e-3
    rerr = np.abs(R - Rstar).max(axis=(1, 2))
    report.append((name, mode, float(short.max()), float(lerr.max()), float(rerr[sep].max()) if sep.any() else None,
                   float(short[sep].max()) if sep.any() else None, int((path == 2).sum()), len(H)))
    assert orth.max() <= ORTHO, (name, mode, orth.max())
    # (allow_reflection on a singular H: the sign of det H is rounding, and either orientation is optimal)
    singular = np.abs(np.linalg.det(H)) <= 1e-10 * scale ** 3
    det_ok = (np.abs(det - want_det) <= ORTHO) | (mirror & singular & (np.abs(np.abs(det) - 1.0) <= ORTHO))
    assert det_ok.all(), (name, mode, det[~det_ok])
    double_top = name == "reflect_double_top" and not mirror
    loose = DOUBLE_TOP if double_top else LOOSE
    assert short.max() <= loose, (name, mode, short.max())
    assert short.min() >= -1e-13, (name, mode, short.min())        # nothing beats the optimum
    assert lerr.max() <= max(loose, LAM_LOOSE), (name, mode, lerr.max())
    if sep.any():
        assert short[sep].max() <= TIGHT, (name, mode, short[sep].max())
        assert lerr[sep].max() <= (DOUBLE_TOP_LAM if double_top else TIGHT), (name, mode, lerr[sep].max())
        assert rerr[sep].max() <= (DOUBLE_TOP_R if double_top else R_TIGHT), (name, mode, rerr[sep].max())


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_kabsch_solve_vs_fp64_svd(mode):
    report = []
    failures = []
    for name, (H, gsum) in families().items():
        try:
            check(name, H, None if mode == 2 else gsum, mode, report)
        except AssertionError as e:
            failures.append(str(e))
    print(f"\nmode {mode}: family, max (sigma* - obj)/|H|, max |lam - sigma*|/|H|, max |R - R*| (gap >= 1e-3), "
          "max short (gap >= 1e-3), rank-1 path / n")
    for r in report:
        print("  %-20s %d  %.2e  %.2e  %s  %s  %d/%d" % (r[0], r[1], r[2], r[3], "%.2e" % r[4] if r[4] is not None else "-",
                                                       "%.2e" % r[5] if r[5] is not None else "-", r[6], r[7]))
    assert not failures, failures


def test_kabsch_zero_and_rank1_exact():
    """H = 0 gives R = I and lam = 0 exactly.  Exact rank 1, H = sigma u v^T: every rotation with u R = v is optimal;
    where the rank-1 path answers, R is the smallest one (Rodrigues from u to v) and lam = sigma."""
    rng = np.random.default_rng(7)
    n = 32
    u, v = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[0] = -u[0]                                             # half turn: any axis perpendicular to u
    H = np.concatenate([np.zeros((1, 3, 3)), np.einsum("bi,bj->bij", u, v) * 2.5])
    gsum = np.r_[0.0, np.full(n, 2 * 2.5 * (1 + 1e-12))]
    for mode in (0, 1, 2):
        R, lam, path = solve(H, gsum, mode)
        assert np.array_equal(R[0], np.eye(3)) and lam[0] == 0.0 and path[0] == 2, mode
        uR = np.einsum("bi,bij->bj", u, R[1:])
        assert np.abs(uR - v).max() <= 1e-6, mode                 # objective short by at most |uR - v|^2 / 2
        assert np.abs(lam[1:] - 2.5).max() <= LOOSE * 2.5, mode
        r1 = np.flatnonzero(path[1:] == 2)
        print(f"\nmode {mode}: rank-1 path on {len(r1)} of {n} exact rank-1 matrices")
        assert np.abs(uR[r1] - v[r1]).max(initial=0.0) <= 1e-13, mode
        assert np.abs(lam[1:][r1] - 2.5).max(initial=0.0) <= 1e-13 * 2.5, mode
        for i in r1[r1 > 0]:
            if np.linalg.det(R[i + 1]) < 0:
                continue                                     # (allow_reflection took -H: -Rodrigues(u -> -v))
            c = u[i] @ v[i]
            w = np.cross(u[i], v[i])
            K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            Rc = c * np.eye(3) + K + np.outer(w, w) / (1 + c)
            assert np.abs(R[i + 1] - Rc.T).max() <= 1e-12, (mode, i)


def test_kabsch_tight_newton_start():
    """Newton's start at (or a few ulps under) the root: gsum = 2 sigma* (1 - k eps), as Y = X R exactly makes it."""
    rng = np.random.default_rng(11)
    n = 48
    H = from_sv(rng, np.sort(rng.random((n, 3)) + 0.05, axis=1)[:, ::-1])
    _, sig, _, frob = reference(H, False)
    for k in (0, 1, 4):
        R, lam, path = solve(H, 2 * sig * (1 - k * EPS), 0)
        obj = np.einsum("bij,bij->b", R, H)
        assert (path == 0).all()
        assert ((sig - obj) / frob).max() <= TIGHT, k
        assert (np.abs(lam - sig) / frob).max() <= TIGHT, k

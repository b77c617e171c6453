"""The ICP kernel of one workgroup per pair comes in two instantiations (icp.hip, icp_kernel<..., WIDE>): the general one, and a
narrow one for launches in which every pair's sort key is a coordinate and the moment sums are one running total -- clouds
below kSortDirMinN (1025 points, config 2), or direction keys switched off.  launch_icp_variant picks one by the shape of the
launch; the two must compute the same thing bit for bit where both apply, and the general one must keep serving the clouds
that take direction keys.  Both tests keep the one-workgroup-per-pair launch (no teams: a team launch would take clouds of
more than 1024 points on a GPU with at least twice as many CUs as pairs) with fewer pairs than the GPU holds at once (no
persistent grid, no half-CU workgroups) and at most two passes per pair (no sums per (pass, wave))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, synthetic  # noqa: E402
from icp_flow_amd import utils_icp_pytorch3d as p3d  # noqa: E402

DEV = torch.device("cuda:0")


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def pad(clouds, n):
    """The same clouds in n slots: the extra rows are padding (1e8, 1e8, 1e8, flag 0), as in synthetic.make_batch."""
    out = np.empty((clouds.shape[0], n, 4), np.float32)
    out[:] = np.array([1e8, 1e8, 1e8, 0], np.float32)
    out[:, :clouds.shape[1]] = clouds
    return out


def sort_codes(fixed):
    """The sort key code each pair's fixed cloud takes (choose_sort_code, sortdir.hpp, in numpy; float32 like the kernel):
    0 .. 2 the longest axis, 3 .. 8 a horizontal direction."""
    c1, s1, c2 = np.float32(0.9238795), np.float32(0.3826834), np.float32(0.7071067)
    dirs = [(c1, s1), (c2, c2), (s1, c1), (-s1, c1), (-c2, c2), (-c1, s1)]
    out = []
    for rows in fixed:
        q = rows[rows[:, 3] > 0, :3].astype(np.float32)
        lo, hi = q.min(0), q.max(0)
        e = hi - lo
        legacy = 0 if (e[0] >= e[1] and e[0] >= e[2]) else (1 if e[1] >= e[2] else 2)
        if len(q) < 1025:
            out.append(legacy)
            continue
        c = np.float32(0.5) * (lo + hi)
        R = np.float32(0.5) * np.sqrt(np.float32((e * e).sum())) + np.float32(0.05)
        inv = np.float32(1.0) / max(np.float32(0.1), np.float32(2.0) * R / np.float32(512))
        d = q - c
        keys = [d[:, 0], d[:, 1], d[:, 2]] + [(uy * d[:, 1].astype(np.float64) + (ux * d[:, 0])).astype(np.float32) for ux, uy in dirs]
        score = []
        for k in keys:
            n = np.bincount(np.clip(((k + R) * inv).astype(np.int64), 0, 511), minlength=512).astype(np.int64)
            score.append(int((n[n > 1] ** 2).sum()))
        best = min(range(9), key=lambda j: (score[j], j))
        out.append(best if score[best] < score[legacy] and score[best] * 10 <= score[legacy] * 9 else legacy)
    return np.array(out)


def test_narrow_and_wide_kernels_agree_on_the_same_clouds():
    """Config 2's clouds (1024 points) in 1024 slots run the narrow kernel; the same clouds in 1100 slots run the general one
    (a launch of that width may have direction keys), on the same sorted inputs -- the fixed clouds are below kSortDirMinN, so
    every pair still sweeps along a coordinate.  The ICP alone (icpflow_icp): transforms, rmse and every iteration's record
    bit for bit."""
    S, D, _ = synthetic.make_batch(64, 1024, seed=0)
    res = []
    for n in (1024, 1100):
        s, d = G(pad(S, n)), G(pad(D, n))
        with _lib.options(no_teams=True):
            res.append(p3d.iterative_closest_point(s, d, max_iterations=50))
    a, b = res
    assert torch.equal(a.RTs.R, b.RTs.R) and torch.equal(a.RTs.T, b.RTs.T) and torch.equal(a.rmse, b.rmse)
    assert len(a.t_history) == len(b.t_history) > 1
    for h1, h2 in zip(a.t_history, b.t_history):
        assert torch.equal(h1.R, h2.R) and torch.equal(h1.T, h2.T)


def test_direction_keys_just_above_the_threshold():
    """1100-point box shells whose heading is along x or y (a face across the longest axis: the clouds the direction keys were
    made for): most of them sort along a direction key, and the launch takes the general kernel; with ICPFLOW_OPT_NO_DIR_KEYS
    every pair sorts along its longest axis and the same launch takes the narrow kernel, two passes of one running sum.  The
    searches are exact under either key, so the iteration count is the same and the transforms differ at most in the order of
    the fp64 sums (test_gpu_fullsize.py, direction keys).  Had the narrow kernel been chosen for the clouds sorted along a
    direction, it would search them along z: other neighbours, other transforms."""
    n, B = 1100, 128
    S, D, _ = synthetic.make_batch(B, n, seed=11)
    for k in range(B):
        r = np.random.default_rng(700 + k)
        ext = np.array([r.uniform(2.5, 5.0), r.uniform(1.2, 2.2), r.uniform(1.0, 2.0)])
        pts = synthetic._shell_points(r, ext, n)
        if k % 2:
            pts = pts[:, [1, 0, 2]]
        c = np.array([r.uniform(-30, 30), r.uniform(-30, 30), 0.8])
        t = np.array([r.uniform(-1, 1), r.uniform(-1, 1), 0.0])
        S[k, :, :3] = (pts + c).astype(np.float32); S[k, :, 3] = 1.0
        D[k, :, :3] = (pts + c + t + r.normal(0, 0.01, pts.shape)).astype(np.float32); D[k, :, 3] = 1.0
    assert (sort_codes(D) >= 3).mean() >= 0.5                      # the case the direction keys exist for
    s, d = G(S), G(D)
    with _lib.options(no_teams=True, no_dir_keys=True):
        narrow = p3d.iterative_closest_point(s, d, max_iterations=50)
    with _lib.options(no_teams=True):
        wide = p3d.iterative_closest_point(s, d, max_iterations=50)
    assert len(narrow.t_history) == len(wide.t_history) > 1
    p = S[:, :, :3].astype(np.float64)
    moved = [np.einsum("bnj,bjk->bnk", p, r.RTs.R.cpu().numpy().astype(np.float64)) + r.RTs.T.cpu().numpy()[:, None].astype(np.float64)
             for r in (narrow, wide)]
    assert np.abs(moved[0] - moved[1]).max() < 1e-9
    same = (narrow.RTs.R == wide.RTs.R).flatten(1).all(1) & (narrow.RTs.T == wide.RTs.T).all(1)
    assert same.float().mean().item() >= 0.99
    for _ in range(2):                                              # and from run to run the same bits
        with _lib.options(no_teams=True):
            again = p3d.iterative_closest_point(s, d, max_iterations=50)
        assert torch.equal(again.RTs.R, wide.RTs.R) and torch.equal(again.RTs.T, wide.RTs.T)

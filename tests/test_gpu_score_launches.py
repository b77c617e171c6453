"""The scoring launches behind the occupancy pre-bound (nn.hip launch_sweep_score_pruned): the ring-level counts of the scans 2 .. 11
are taken beside candidate 0's scans, and the launch of those ten scans is laid out by (pair, query block, survivor slot) -- every
workgroup compares for itself, only the scans that go on are scanned.  Nothing but results here: on every shape at which that launch
takes another path, `hist_icp` (transforms and iteration count) and `estimate_init_pose` are bit for bit those of the sweeps without
the grids (ICPFLOW_OPT_NO_SCORE_PREBOUND) and of every scan run to its end (ICPFLOW_OPT_NO_SCORE_PRUNE)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, synthetic, utils_hist, utils_match  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")
VARIANTS = ({"no_score_prebound": True}, {"no_score_prune": True})


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def C(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _equal(x, y):
    """torch.equal, or the same bits (a pair with an empty cloud may come out as NaN: the same NaN)."""
    return torch.equal(x, y) or torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _same_under_every_variant(a, s, d, rows=None, init=True, **opts):
    """hist_icp and (init) estimate_init_pose with the default scoring, then under each variant: torch.equal (on `rows`, or everywhere)."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    with _lib.options(**opts):
        T1, it1 = utils_match.hist_icp(a, s, d, return_iterations=True)
        init1 = utils_hist.estimate_init_pose(a, s, d) if init else None
    out = {}
    for v in VARIANTS:
        with _lib.options(**opts, **v):
            T0, it0 = utils_match.hist_icp(a, s, d, return_iterations=True)
            init0 = utils_hist.estimate_init_pose(a, s, d) if init else None
        assert int(it0) == int(it1), v
        assert _equal(pick(T0), pick(T1)), v
        assert not init or _equal(pick(init0), pick(init1)), v
        out[tuple(v)] = init0
    return T1, it1, init1, out[("no_score_prune",)]


def _backward_winner_pair(N, seed):
    """The "two backward winners" pair of test_gpu_fullsize.py: src role a 100-point patch P and a tight 300-point clump K three metres
    above it; dst role ten jittered copies of P moved by t1 = (-0.3, 0.4, 0) and 20 points of K moved by t0 = (0.4, 0.4, 0).  The
    vote's highest peak is t0; t1 has the larger forward mean and by far the smallest backward mean: it wins through its backward scan."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(0, 1, 100), rng.uniform(0, 1, 100), rng.uniform(-0.01, 0.01, 100)], 1)
    K = np.array([0.5, 0.5, 3.0]) + rng.uniform(-0.01, 0.01, (300, 3))
    t0, t1 = np.array([0.4, 0.4, 0.0]), np.array([-0.3, 0.4, 0.0])
    A = np.concatenate([P, K])
    Cc = np.concatenate([np.repeat(P, 10, 0) + t1 + rng.normal(0, 0.003, (1000, 3)), K[:20] + t0])
    S = np.full((N, 4), 1e8, np.float32); S[:, 3] = 0
    D = S.copy()
    S[:len(A), :3] = A + 10.0; S[:len(A), 3] = 1
    D[:len(Cc), :3] = Cc + 10.0; D[:len(Cc), 3] = 1
    return S, D


def _scans_that_cannot_end(a, S, D):
    """From the oracle alone: per pair candidate 0's translation and the number of scans of the OTHER candidates whose mean does not
    exceed candidate 0's score.  No bound may end such a scan (a bound only ends a scan whose mean provably exceeds that score): it
    survives the pre-bound and is scanned.  (Whichever cloud takes which role, the two means of a candidate are the same two.)"""
    _, aux = rp.estimate_init_pose_batch(a, C(S), C(D), return_aux=True)
    cand = aux["candidates"].numpy().astype(np.float64)
    B, K = cand.shape[:2]
    must = np.zeros(B, int)
    for b in range(B):
        p, q = S[b, S[b, :, 3] > 0, :3].astype(np.float64), D[b, D[b, :, 3] > 0, :3].astype(np.float64)
        if len(p) == 0 or len(q) == 0:
            continue
        means = []
        for k in range(K):
            dist = np.sqrt((((p + cand[b, k])[:, None, :] - q[None, :, :]) ** 2).sum(-1))
            means.append((dist.min(1).mean(), dist.min(0).mean()))
        s0 = min(means[0]) * (1 - 1e-6)   # (the oracle's means are fp32 sums: a scan counts only where it is clearly not above)
        must[b] = sum(int(f <= s0) + int(w <= s0) for f, w in means[1:])
    return cand[:, 0], must


@pytest.mark.parametrize("rows,width", [(300, 1024), (200, 1024), (300, 300)])
def test_query_blocks_beyond_the_cloud(rows, width):
    """8 pairs x 300 points in a grid of four query blocks (rows in blocks 0 and 1, a short second block, two blocks beyond every
    cloud), x 200 points (ONE block with rows, three beyond), and x 300 unpadded (two blocks, none beyond)."""
    S, D, _ = synthetic.make_batch(8, rows, seed=1)
    pad = np.full((8, width, 4), 1e8, np.float32); pad[:, :, 3] = 0
    S1, D1 = pad.copy(), pad.copy()
    S1[:, :rows], D1[:, :rows] = S, D
    a = rp.default_args(max_points=width, icp_max_iterations=30)
    T1, it1, _, _ = _same_under_every_variant(a, G(S1), G(D1))
    assert int(it1) > 0 and bool(torch.isfinite(T1).all())


def test_five_query_blocks_survivors_and_a_pick_beside_candidate_0():
    """8 pairs x 1100 points (five query blocks, the last one short), two of them pairs whose winner is NOT candidate 0 and wins
    through its backward scan.  From the oracle: at least two scans of the other candidates cannot be ended by any bound, and from
    the run with every scan to its end: the picks of those two pairs differ from candidate 0's translation."""
    N = 1100
    S, D, _ = synthetic.make_batch(8, N, seed=41, ragged=True, n_min=300)
    for b, seed in ((2, 0), (5, 1)):
        S[b], D[b] = _backward_winner_pair(N, seed)
    a = rp.default_args(max_points=N, icp_max_iterations=50)
    cand0, must = _scans_that_cannot_end(a, S, D)
    print("scans of the other candidates that no bound can end, per pair:", must.tolist())
    assert must.sum() >= 2
    _, _, init1, init_full = _same_under_every_variant(a, G(S), G(D))
    t_full = init_full.cpu().numpy()[:, :3, 3].astype(np.float64)
    off0 = np.abs(t_full - cand0).max(1) > 0.05   # (candidates are bins of 0.1 m apart or more)
    print("pairs whose pick is not candidate 0:", np.flatnonzero(off0).tolist())
    assert off0[2] and off0[5]
    assert np.array_equal(init1.cpu().numpy(), rp.estimate_init_pose(a, C(S), C(D)).numpy())


def test_ragged_batch_padded_to_four_query_blocks():
    S, D, _ = synthetic.make_batch(24, 1024, seed=9, ragged=True, n_min=40)
    a = rp.default_args(max_points=1024, icp_max_iterations=30)
    _same_under_every_variant(a, G(S), G(D))


def test_an_empty_cloud_and_three_runs_in_a_row():
    """One pair with an empty cloud among ordinary ones; the same batch three times in a row: the same bits every time (the launch
    leaves no counter or record behind that the next call would read), then the variants."""
    S, D, _ = synthetic.make_batch(12, 600, seed=23, ragged=True, n_min=50)
    S[4, :, :3] = 1e8; S[4, :, 3] = 0
    a = rp.default_args(max_points=600, icp_max_iterations=30)
    s, d = G(S), G(D)
    runs = [utils_match.hist_icp(a, s, d, return_iterations=True) for _ in range(3)]
    inits = [utils_hist.estimate_init_pose(a, s, d) for _ in range(3)]
    for T, it in runs[1:]:
        assert int(it) == int(runs[0][1]) and _equal(T, runs[0][0])
    for i in inits[1:]:
        assert _equal(i, inits[0])
    T1, _, init1, _ = _same_under_every_variant(a, s, d)
    assert _equal(T1, runs[0][0]) and _equal(init1, inits[0])
    # (long clouds against short ones, where the sweeps share a scan between workgroups: the same three runs)
    S2, D2, _ = synthetic.make_batch(10, 2304, seed=5, ragged=True, n_min=40)
    D2[7, :, :3] = 1e8; D2[7, :, 3] = 0
    a2 = rp.default_args(max_points=2304, icp_max_iterations=20)
    s2, d2 = G(S2), G(D2)
    first = utils_match.hist_icp(a2, s2, d2)
    for _ in range(2):
        assert _equal(utils_match.hist_icp(a2, s2, d2), first)
    T2, _, _, _ = _same_under_every_variant(a2, s2, d2)
    assert _equal(T2, first)


def test_masked_pairs_do_not_disturb_their_neighbours():
    """options.d_pair_active with two pairs out of the batch (their clouds still in place): the scoring runs for every row, the
    pairs in the batch come out bit for bit under every variant.  (hist_icp only: estimate_init_pose refuses a mask.)"""
    S, D, _ = synthetic.make_batch(16, 700, seed=77, ragged=True, n_min=60)
    keep = np.ones(16, dtype=bool); keep[[3, 10]] = False
    a = rp.default_args(max_points=700, icp_max_iterations=40)
    rows = torch.from_numpy(np.flatnonzero(keep)).to(DEV)
    T1, it1, _, _ = _same_under_every_variant(a, G(S), G(D), rows=rows, init=False, pair_active=G(keep.astype(np.uint8)))
    assert int(it1) > 0 and bool(torch.isfinite(T1[rows]).all())


def _many_good_candidates_pair(N, seed):
    """src role: a 100-point patch P.  dst role: P twice with 2 cm of noise, moved by t0 -- the highest peak of the vote -- and exact
    copies of P moved by four other translations and by none, every translation a millimetre above a bin's left edge (the candidates
    are left edges).  The forward scans of the four other peaks and of the zero translation land on their copies: means of a
    millimetre or two, below candidate 0's (its copies are noisy).  Five scans that no bound can end; the copy at x = 0.8 fits best."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(0, 1, 100), rng.uniform(0, 1, 100), rng.uniform(-0.01, 0.01, 100)], 1)
    eps = 0.001
    t0 = np.array([eps, 0.8 + eps, eps])
    # (residuals of 0.2 mm at x = 0.8, 1 mm at the other peaks, 2 mm at the zero translation: ONE best candidate, by a clear margin)
    others = [np.array([x + e, e, e]) for x, e in ((-1.6, eps), (-0.8, eps), (0.8, 0.2 * eps), (1.6, eps))] + [np.full(3, 2 * eps)]
    Cc = np.concatenate([np.repeat(P, 2, 0) + t0 + rng.normal(0, 0.02, (200, 3))] + [P + t for t in others])
    S = np.full((N, 4), 1e8, np.float32); S[:, 3] = 0
    D = S.copy()
    S[:len(P), :3] = P + 10.0; S[:len(P), 3] = 1
    D[:len(Cc), :3] = Cc + 10.0; D[:len(Cc), 3] = 1
    return S, D


def test_more_surviving_scans_in_a_pair_than_survivor_slots():
    """16 pairs with five candidates as good as candidate 0 or better: more scans go on in every pair than the launch has slots of a
    workgroup per query block (four): the fifth takes a slot whose workgroup scans the query blocks of its scan in turn.  The count is asserted from the oracle, not assumed."""
    N = 704
    pairs = [_many_good_candidates_pair(N, seed) for seed in range(16)]
    S, D = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    a = rp.default_args(max_points=N, icp_max_iterations=30)
    _, must = _scans_that_cannot_end(a, S, D)
    print("scans of the other candidates that no bound can end, per pair:", must.tolist())
    assert (must >= 5).sum() >= 12
    _, _, init1, _ = _same_under_every_variant(a, G(S), G(D))
    want = rp.estimate_init_pose(a, C(S), C(D)).numpy()   # (an independent reference for the picks among scans that all went on)
    assert np.array_equal(init1.cpu().numpy(), want)
    assert np.allclose(want[:, :3, 3], [0.8, 0.0, 0.0], atol=1e-6)

"""hist_icp's ICP launch picks its own initial poses (icp.hip icp_pair's prologue, scorepick.hpp; api.hip pick_in_icp): where the
scoring ran as sorted sweeps and ONE speculative launch gives every pair one workgroup, no score_pick_kernel runs -- wave 0 of
the pair's workgroup picks, the other waves stage the fixed cloud meanwhile.  The library still offers the same registration
unfolded: the initial-pose entry point (which keeps score_pick_kernel) followed by apply_icp from its poses.  For pairs that
hist_icp does not swap (n_src <= n_dst) the two must agree bit for bit, and the initial poses must be those of a NumPy
restatement of the pick (candidates from the library's own vote and peak search; means, first arg-min, NaN rule restated).

The restatement sums exact fp32 point differences in fp64 and rounds once, where the kernels round every fma: its means can
differ from the library's in the last bits (about 1e-7 relative), so it is only asked about pairs whose two best scores lie
further apart than 1e-4 relative -- or tie exactly, on clouds built on a binary lattice where every sum is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, synthetic, utils_hist, utils_icp, utils_match  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")
PAD = np.array([1e8, 1e8, 1e8, 0], np.float32)


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same(a, b):
    """bit for bit, NaN equal to NaN (an empty cloud registers to NaN on either path)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def composition(a, s, d):
    """The registration unfolded: score_pick_kernel's poses, then ICP + roll-back from them."""
    init = utils_hist.estimate_init_pose(a, s, d)
    T, it = utils_icp.apply_icp(a, s, d, init, return_iterations=True)
    return init, T, it


def ragged(lens, N, seed):
    """Pairs of the given (n_src, n_dst), padded to N (synthetic.make_pair; 0 = an empty cloud)."""
    S, D = np.empty((len(lens), N, 4), np.float32), np.empty((len(lens), N, 4), np.float32)
    for k, (ns, nd) in enumerate(lens):
        S[k], D[k], _ = synthetic.make_pair(k, max(ns, 1), max(nd, 1), N, seed)
        S[k, ns:], D[k, nd:] = PAD, PAD
    return S, D


# ------------------------------------------------------------------------------------------------ the pick, restated
def candidates(a, bins):
    """The six candidate translations per pair from the vote's bins, by the library's own peak search (utils_hist.py:78-83)."""
    ex, ey, ez = (e.numpy() for e in utils_hist.bin_edges(a))
    B, (Lx, Ly, Lz) = bins.shape[0], (len(ex), len(ey), len(ez))
    _, idx = utils_hist.topk_nms(bins.to(torch.float32).reshape(B, Lx, Ly, Lz))
    f = idx.cpu().numpy()
    sh = np.float32(a.thres_dist // 2)
    cand = np.zeros((B, 6, 3), np.float32)
    cand[:, :5, 0], cand[:, :5, 1], cand[:, :5, 2] = ex[f // Lz // Ly % Lx] + sh, ey[f // Lz % Ly] + sh, ez[f % Lz] + sh
    return cand


def nn_total(q, t):
    """sum over the queries q of the distance to the nearest target t: fp32 differences, squared and summed in fp64, rounded once"""
    if len(q) == 0 or len(t) == 0:
        return 0.0
    q, t = q.astype(np.float32), t.astype(np.float32)
    d2 = np.zeros((len(q), len(t)))
    for k in range(3):
        d2 += (q[:, None, k] - t[None, :, k]).astype(np.float64) ** 2
    d = np.sqrt(d2.min(1).astype(np.float32).astype(np.float64)).astype(np.float32)
    return float(d.astype(np.float64).sum())


def restated_pick(cand, src, dst):
    """-> (index of the picked candidate, the six scores): score_k = min(mean fwd, mean bwd) in fp32, the FIRST minimum wins, a
    NaN score never beats the best so far (candidate 0 stands when all are NaN)."""
    p, q = src[src[:, 3] > 0, :3], dst[dst[:, 3] > 0, :3]
    na, nc = np.float32(len(p)), np.float32(len(q))
    sc = np.empty(6, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(6):
            moved = p + cand[k]                                          # fp32, as the scans form src + t
            fwd = np.float32(nn_total(moved, q)) / na
            bwd = np.float32(nn_total(q, moved)) / nc
            sc[k] = bwd if np.isnan(fwd) else (fwd if np.isnan(bwd) else min(fwd, bwd))   # fminf
    pick, best = 0, sc[0]
    for k in range(1, 6):
        if sc[k] < best:
            pick, best = k, sc[k]
    return pick, sc


def pose_of(t):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = t
    return T


def decided(sc):
    """the two best scores tie exactly or lie 1e-4 (relative) apart: the restatement's rounding cannot change the pick"""
    s = np.sort(sc[~np.isnan(sc)])
    return len(s) < 2 or s[0] == s[1] or s[1] - s[0] > 1e-4 * max(abs(s[1]), 1e-3)


def check_against_restatement(a, S, D, init, rows=None):
    bins = torch.zeros((len(S), int(np.prod([len(e) for e in utils_hist.bin_edges(a)]))), dtype=torch.int32, device=DEV)
    with _lib.options(vote_bins=bins):
        again = utils_hist.estimate_init_pose(a, G(S), G(D))
    assert same(again, init)
    cand = candidates(a, bins)
    asked = 0
    for b in (range(len(S)) if rows is None else rows):
        pick, sc = restated_pick(cand[b], S[b], D[b])
        if not decided(sc):
            continue
        asked += 1
        assert np.array_equal(init[b].cpu().numpy(), pose_of(cand[b, pick])), (b, pick, sc)
    return asked


# ------------------------------------------------------------------------------------------------ every block size
@pytest.mark.parametrize("N", [64, 65, 256, 257, 513, 769, 1024])
def test_folded_registration_equals_the_composition(N):
    """Five full pairs per width: 256, 512, 768 and 1024 threads per workgroup.  (Up to 512 points the scoring runs as all-pairs
    scans and hist_icp keeps the kernel; above it the ICP launch picks.)  hist_icp and hist_icp_eval against the composition,
    the composition's initial poses against the restatement."""
    S, D, _ = synthetic.make_batch(5, N, seed=300 + N)
    a = rp.default_args(max_points=N, icp_max_iterations=50)
    s, d = G(S), G(D)
    init, T, it = composition(a, s, d)
    Tf, itf = utils_match.hist_icp(a, s, d, return_iterations=True)
    assert int(itf) == int(it) and same(Tf, T)
    Te, ev, ite = utils_match.hist_icp_eval(a, s, d, return_iterations=True)
    assert int(ite) == int(it) and same(Te, T)
    for got, want in zip(ev, utils_match.match_eval(a, s, d, T)):
        assert same(got, want)
    assert check_against_restatement(a, S, D, init) >= 3


# ------------------------------------------------------------------------------------------------ ragged, masked, reruns
LENS = [(1024, 1024), (700, 1000), (1, 900), (0, 800), (513, 513), (65, 769)]


def test_ragged_lengths_an_empty_and_a_one_point_cloud():
    """Ragged pairs, none swapped, among them an empty moving cloud (its means are 0 / 0: NaN -- candidate 0 stands, the
    registration is NaN on both paths) and a one-point cloud; a rerun on the same workspace and a run on a second stream."""
    S, D = ragged(LENS, 1024, seed=41)
    a = rp.default_args(max_points=1024, icp_max_iterations=50)
    s, d = G(S), G(D)
    init, T, it = composition(a, s, d)
    Tf, itf = utils_match.hist_icp(a, s, d, return_iterations=True)
    assert int(itf) == int(it) and same(Tf, T)
    Te, _, ite = utils_match.hist_icp_eval(a, s, d, return_iterations=True)
    assert int(ite) == int(it) and same(Te, T)
    # (pair 3, the empty cloud: every forward mean is NaN and the six scores are equal whatever the backward scans of an empty
    # target set report -- no score beats candidate 0, which the restatement is asked about like any other pair)
    assert check_against_restatement(a, S, D, init) >= 4
    T2, it2 = utils_match.hist_icp(a, s, d, return_iterations=True)              # the same workspace again
    assert int(it2) == int(it) and same(T2, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        T3, it3 = utils_match.hist_icp(a, s, d, return_iterations=True)          # a workspace of its own on another stream
    side.synchronize()
    assert int(it3) == int(it) and same(T3, T)


def test_a_masked_pair():
    """options.d_pair_active with one pair out of the batch, its clouds still in place: the other pairs register as the batch
    made of them alone does unfolded (one workgroup per pair either way: the same sums), and the masked pair's workgroup,
    which picks and leaves, disturbs nothing -- twice on the same workspace."""
    S, D = ragged([(1024, 1024), (700, 1000), (900, 950), (513, 600), (800, 1024)], 1024, seed=52)
    keep = np.array([1, 1, 0, 1, 1], bool)
    a = rp.default_args(max_points=1024, icp_max_iterations=50)
    _, T, it = composition(a, G(S[keep]), G(D[keep]))
    for _ in range(2):
        with _lib.options(pair_active=G(keep.astype(np.uint8))):
            Tf, itf = utils_match.hist_icp(a, G(S), G(D), return_iterations=True)
        assert int(itf) == int(it) and same(Tf[G(keep)], T)


def test_persistent_grid_one_workgroup_picks_for_several_pairs():
    """513 pairs x 800 points: more pairs than the GPU holds 1024-thread workgroups, a persistent grid whose workgroups draw
    further pairs by ticket and pick for each of them."""
    S, D, _ = synthetic.make_batch(513, 800, seed=7)
    a = rp.default_args(max_points=800, icp_max_iterations=50)
    s, d = G(S), G(D)
    _, T, it = composition(a, s, d)
    Tf, itf = utils_match.hist_icp(a, s, d, return_iterations=True)
    assert int(itf) == int(it) and same(Tf, T)


# ------------------------------------------------------------------------------------------------ hand-made picks
def lattice(rng, n):
    """n distinct points on the lattice of 1/64 m in a 3 x 2 x 1 m box around (8, -5, 0.5): every coordinate, translation and
    squared distance below is exact in fp32"""
    cells = rng.choice(192 * 128 * 64, size=n, replace=False)
    p = np.stack([cells // (128 * 64), cells // 64 % 128, cells % 64], 1).astype(np.float32) / np.float32(64)
    return p + np.array([8, -5, 0], np.float32)


def padded(points, N=1024):
    out = np.tile(PAD, (N, 1))
    out[:len(points), :3] = points
    out[:len(points), 3] = 1
    return out


T1, T2 = np.array([0.5, 0.25, 0], np.float32), np.array([-0.75, 0.5, 0], np.float32)


def hand_made():
    """Bins of 1/8 m (edges on the lattice: a candidate IS the translation it stands for).
    0: an exact tie -- dst holds src + T1 and src + T2 whole, both forward means are exactly 0; T1's bin gets more votes (half of
       src once more, 1/64 m beside), so T1 is the earlier candidate and must win.
    1: dst = src + T1: candidate 0 scores exactly 0 and every other scan is pruned (+inf).
    2: the same, swapped by hist_icp (n_src > n_dst): the pick runs with the roles exchanged and finds -T1."""
    rng = np.random.default_rng(5)
    P = lattice(rng, 400)
    S = [padded(P[:300]), padded(P[:300]), padded(P)]
    D = [padded(np.concatenate([P[:300] + T1, P[:300] + T2, P[:150] + T1 + np.array([1 / 64, 0, 0], np.float32)])),
         padded(P[:300] + T1), padded(P[:300] + T1)]
    return np.stack(S), np.stack(D)


def test_hand_made_picks():
    """Under the picked pose the mean NN error is exactly 0, the ICP cannot lower it and the roll-back returns the initial pose:
    hist_icp's result shows the pick itself (for the swapped pair its exact inverse)."""
    S, D = hand_made()
    a = rp.default_args(max_points=1024, icp_max_iterations=50, thres_dist=0.125, translation_frame=2.0)
    s, d = G(S), G(D)
    # the restatement, on the roles hist_icp gives the clouds (pair 2 swapped)
    Sr, Dr = S.copy(), D.copy()
    Sr[2], Dr[2] = D[2], S[2]
    bins = torch.zeros((3, int(np.prod([len(e) for e in utils_hist.bin_edges(a)]))), dtype=torch.int32, device=DEV)
    with _lib.options(vote_bins=bins):
        Tf, itf = utils_match.hist_icp(a, s, d, return_iterations=True)
    cand = candidates(a, bins)
    picks = [restated_pick(cand[b], Sr[b], Dr[b]) for b in range(3)]
    # pair 0: T1 in front of T2 among the candidates, both scores exactly 0, the first wins
    i1 = int(np.nonzero((cand[0] == T1).all(1))[0][0])
    i2 = int(np.nonzero((cand[0] == T2).all(1))[0][0])
    assert i1 < i2 and picks[0][1][i1] == 0 and picks[0][1][i2] == 0 and picks[0][0] == i1
    assert picks[1][0] == 0 and (cand[1, 0] == T1).all() and picks[1][1][0] == 0
    assert (cand[2, picks[2][0]] == -T1).all() and picks[2][1][picks[2][0]] == 0
    got = Tf.cpu().numpy()
    assert np.array_equal(got[0], pose_of(T1)) and np.array_equal(got[1], pose_of(T1))
    assert np.array_equal(got[2], pose_of(T1))                                   # the inverse of [I | -T1]
    # and the unswapped pairs against the composition
    init, T, it = composition(a, s[:2], d[:2])
    assert np.array_equal(init.cpu().numpy(), np.stack([pose_of(T1), pose_of(T1)]))
    T01, it01 = utils_match.hist_icp(a, s[:2], d[:2], return_iterations=True)
    assert int(it01) == int(it) and same(T01, T)

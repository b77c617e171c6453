"""The vote's inner loop (hist.hip vote_range: a ring of four targets in flight, trips of four, the rest of a window on its own,
votes into LDS under the exec mask) on the smallest inputs that sit on its seams, bit for bit against the oracle's vote
(hist_cuda_core.cuh:40-60): the bins the registration path exports (`_lib.options(vote_bins=...)`) through estimate_init_pose and
through hist_icp, and the same bins again from a call on another stream.

What each input is -- window lengths per wave, shares, tile seams -- is asserted on the CPU by tests/test_vote_loop_cases.py.  Which
kernel a case reaches on a 256-CU device is recorded in COVERAGE.md (checked once under a kernel trace); the shapes below are taken
from launch_hist_vote_sorted's policy so that every instantiation is launched, the test itself does not restate it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, utils_hist, utils_match  # noqa: E402
from icp_flow_amd import hist as hip_hist  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

import vote_loop_cases as vc  # noqa: E402

DEV = torch.device("cuda:0")


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def C(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _wide():
    pairs = [vc.wide_pair(1500, s) for s in (1, 2)]
    return vc.batch(pairs, 1536)


# name: (clouds, translation_frame, thres_dist).  The batch shapes pick the kernel (COVERAGE.md); the padded widths hold few valid rows.
CASES = {
    # one wave, k = 0 .. 13 and longer targets in its window, whole windows per wave: 1024 rows per workgroup (few waves in the batch)
    "windows_22x256_tf2_pow2_lds": (lambda: vc.window_batch(22, 256), 2.0, 0.1),
    "windows_22x256_tf1p5_general_lds": (lambda: vc.window_batch(22, 256), 1.5, 0.1),
    "windows_22x256_extent_4e18_plain_division_lds": (lambda: vc.window_batch(22, 256, 1e18), 2e18, 1e17),
    "windows_22x256_tf8_pow2_global": (lambda: vc.window_batch(22, 256), 8.0, 0.1),
    "windows_22x256_tf3p34_general_global": (lambda: vc.window_batch(22, 256), 3.34, 0.1),
    "windows_22x256_extent_16e18_plain_division_global": (lambda: vc.window_batch(22, 256, 1e18), 8e18, 1e17),
    # ... a quarter of a window per wave (four waves per 64 rows), alone and behind the grids and the axis sort in one launch
    "windows_22x1024_tf2_quarters": (lambda: vc.window_batch(22, 1024), 2.0, 0.1),
    "windows_22x1024_tf1p5_quarters": (lambda: vc.window_batch(22, 1024), 1.5, 0.1),
    # ... half a window per wave, or whole windows on 256 rows per workgroup
    "windows_128x1023_tf2_halves": (lambda: vc.window_batch(128, 1023), 2.0, 0.1),
    # ... whole windows, 512 rows per workgroup
    "windows_257x1023_tf2_512_rows": (lambda: vc.window_batch(257, 1023), 2.0, 0.1),
    # tiles: 1023, 1024, 1025 and 2049 targets, windows across the seams
    "seams_4x2112_tf2": (vc.seam_batch, 2.0, 0.1),
    "seams_4x2112_tf13p36_global": (vc.seam_batch, 13.36, 0.1),
    # differences on the box's upper face: the overflow row behind a pair's bins, the last pair's limit
    "faces_5x300_tf2": (lambda: vc.face_batch(2.0)[0], 2.0, 0.1),
    "faces_5x300_tf13p36_global": (lambda: vc.face_batch(13.36)[0], 13.36, 0.1),
    # the composite key: slab windows
    "wide_2x1536_tf2": (_wide, 2.0, 0.1),
}

_oracle = {}


def _case(name):
    """clouds, args, edges and the oracle's bins [B, L] (int64) for the roles of both entry points: computed once per case"""
    if name not in _oracle:
        make, tf, th = CASES[name]
        S, D = make()
        a = rp.default_args(max_points=S.shape[1], translation_frame=tf, thres_dist=th, icp_max_iterations=2)
        ex, ey, ez = rp.bin_edges(a)
        lens = (len(ex), len(ey), len(ez))
        want = {}
        sw = (S[:, :, 3] > 0).sum(1) > (D[:, :, 3] > 0).sum(1)                       # utils_match.py:142
        for entry in ("estimate_init_pose", "hist_icp"):
            src, dst = S.copy(), D.copy()
            if entry == "hist_icp":
                src[sw], dst[sw] = D[sw], S[sw]
            if entry == "hist_icp" and not sw.any():
                want[entry] = want["estimate_init_pose"]
                continue
            w = rp.hist(C(dst), C(src), ex.min(), ey.min(), ez.min(), ex.max(), ey.max(), ez.max(), *lens)
            want[entry] = w.numpy().reshape(len(S), -1).astype(np.int64)
        _oracle[name] = (S, D, a, lens, want)
    return _oracle[name]


def _bins(entry, a, s, d, B, L):
    bins = torch.full((B, L), -1, dtype=torch.int32, device=DEV)      # uint32 on the device, every bin overwritten
    with _lib.options(vote_bins=bins):
        (utils_hist.estimate_init_pose if entry == "estimate_init_pose" else utils_match.hist_icp)(a, s, d)
    return bins


@pytest.mark.parametrize("entry", ["estimate_init_pose", "hist_icp"])
@pytest.mark.parametrize("case", list(CASES))
def test_vote_loop_bins_bit_exact(case, entry):
    S, D, a, lens, want = _case(case)
    want = want[entry]
    B, L = len(S), lens[0] * lens[1] * lens[2]
    s, d = G(S), G(D)
    bins = _bins(entry, a, s, d, B, L)
    got = bins.cpu().numpy().view(np.uint32).astype(np.int64)
    print(f"{case} {entry}: {int(want.sum())} votes, {int((got != want).sum())} of {got.size} bins differ")
    assert want.sum() > 0
    if case.startswith("windows"):      # every target inside a window is inside the box for all 64 rows, nothing else is
        ks = [vc.WINDOW_KS[b % len(vc.WINDOW_KS)] for b in range(B)]
        assert want.sum(1).tolist() == [vc.WAVE * k for k in ks]
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} bins differ"
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _bins(entry, a, s, d, B, L)
    side.synchronize()
    assert torch.equal(again, bins)


@pytest.mark.parametrize("tf", [2.0, 13.36])
def test_drop_in_hist_short_clouds_bit_exact(tf):
    """hist_vote_kernel (no z window: a tile's flagged and unflagged rows, all walked), counters in LDS (tf 2.0) and in global memory
    (13.36): clouds of 1, 3, 4, 5 and 257 flagged rows with unflagged ones in between"""
    X, Y = vc.hist_batch()
    a = rp.default_args(max_points=X.shape[1], translation_frame=tf)
    ex, ey, ez = rp.bin_edges(a)
    box = (ex.min(), ey.min(), ez.min(), ex.max(), ey.max(), ez.max(), len(ex), len(ey), len(ez))
    want = rp.hist(C(X), C(Y), *box).numpy()
    assert want.reshape(len(X), -1).sum(1).min() > 0        # even the pair of one row and one target votes
    x, y = G(X), G(Y)
    got = hip_hist.hist(x, y, *box)
    assert np.array_equal(got.cpu().numpy(), want)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = hip_hist.hist(x, y, *box)
    side.synchronize()
    assert torch.equal(again, got)

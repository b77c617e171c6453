"""The cases of tests/test_gpu_vote_loop.py are what they were built for (CPU only): the kernel's z window restated
(vote_loop_cases.wave_windows) gives every wave the window length -- and with it the trips, the rest and the shares -- that the case's
name claims.  No GPU, no library: NumPy on the inputs."""
import numpy as np
import pytest

import vote_loop_cases as vc

F = np.float32


@pytest.mark.parametrize("scale,th", [(1.0, 0.1), (1e18, 1e17)])
@pytest.mark.parametrize("entry", ["estimate_init_pose", "hist_icp"])
def test_window_batch_one_wave_with_exactly_k_targets_between_rows_far_below_and_above(entry, scale, th):
    B = len(vc.WINDOW_KS)
    S, D = vc.window_batch(B, 256, scale)
    min_z, max_z = vc.z_box(th)
    lengths = []
    for b, (rows, targets) in enumerate(vc.roles(S, D, entry)):
        k = vc.WINDOW_KS[b]
        assert len(rows) == vc.WAVE and len(targets) == k + vc.N_BELOW + vc.N_ABOVE      # the 64 rows are the rows under either entry
        assert len(np.unique(rows[:, 2])) == 1                                           # one height
        (r0, r1), = vc.wave_windows(rows, targets, min_z, max_z)                         # one wave
        assert (r0, r1) == (vc.N_BELOW, vc.N_BELOW + k)                                  # r0 > 0: rows below the window
        assert vc.tile_windows(r0, r1, len(targets)) == [(r0, r1)]
        # every target of the window votes (inside the box on all three axes), nothing else does
        inside = np.abs(rows[:, None, 2] - targets[None, :, 2]) < 0.06 * scale        # (the box is 0.1 * scale high on either side)
        assert int(inside.all(0).sum()) == k and int(inside.any(0).sum()) == k
        lengths.append(r1 - r0)
    assert lengths == vc.WINDOW_KS
    # a wave that takes the whole window (SPLIT = 1), half of it, a quarter of it: every residue mod 4, the empty range, one target,
    # and two trips or more with a rest that is no multiple of four
    for split in (1, 2, 4):
        got = [b - a for n in lengths for a, b in vc.shares(vc.N_BELOW, vc.N_BELOW + n, split)]
        assert {n % 4 for n in got} == {0, 1, 2, 3} and 0 in got and 1 in got, (split, sorted(set(got)))
        assert any(vc.trips(n)[0] >= 2 and vc.trips(n)[1] % 4 for n in got), (split, sorted(set(got)))
        assert {vc.trips(n)[1] for n in got} >= set(range(8)), (split, sorted(set(got)))   # every length of the rest, 0 .. 7
    # shares of the short windows: empty ones and single targets (windows of 0, 1, 2, 3 and 5 targets)
    assert {0, 1, 2, 3, 5} <= set(lengths)
    for split in (2, 4):
        short = [b - a for n in (0, 1, 2, 3, 5) for a, b in vc.shares(0, n, split)]
        assert 0 in short and 1 in short and max(short) <= 3


def test_trips_restate_the_loop():
    assert [vc.trips(n) for n in (0, 1, 4, 7, 8, 9, 11, 12, 13, 16)] == [(0, 0), (0, 1), (0, 4), (0, 7), (1, 4), (1, 5), (1, 7), (2, 4), (2, 5), (3, 4)]


@pytest.mark.parametrize("entry", ["estimate_init_pose", "hist_icp"])
def test_seam_batch_windows_cross_the_tile_seams(entry):
    S, D = vc.seam_batch()
    min_z, max_z = vc.z_box()
    for (rows, targets), ny in zip(vc.roles(S, D, entry), vc.SEAM_NY):
        assert len(targets) == ny and len(rows) == ny + 7
        win = vc.wave_windows(rows, targets, min_z, max_z)
        assert all(r1 - r0 >= 8 for r0, r1 in win)                                        # every wave runs trips
        for seam in (1024, 2048):
            if ny > seam:   # a window with targets on both sides of the seam: its last tile-relative range ends at the tile's end,
                            # the next tile's begins at its first row
                cross = [(r0, r1) for r0, r1 in win if r0 < seam < r1]
                assert cross, (ny, seam)
                for r0, r1 in cross:
                    t = vc.tile_windows(r0, r1, ny)
                    assert t[seam // vc.TILE - 1][1] == vc.TILE and t[seam // vc.TILE][0] == 0 and t[seam // vc.TILE][1] >= 1
        assert any(r1 == ny for _, r1 in win)                                             # a window that ends with the last valid row
    # 1025 and 2049: the last tile holds ONE row (whatever lies behind it in LDS is the tile before's)
    assert vc.tile_windows(0, 1025, 1025)[-1] == (0, 1) and vc.tile_windows(0, 2049, 2049)[-1] == (0, 1)


@pytest.mark.parametrize("tf", [2.0, 13.36])
def test_face_batch_quotient_rounds_to_one(tf):
    (S, D), hi = vc.face_batch(tf)
    ex = np.arange(-tf, tf + 0.1 - 1e-8, 0.1).astype(F)
    for b in (1, 2, 4):
        vx = F(D[b, 0, 0]) - F(S[b, 0, 0])
        assert vx == hi < ex[-1] and F(F(vx - ex[0]) / F(ex[-1] - ex[0])) == F(1.0)
    assert len(S) == 5                                                                     # pair 4 is the last: nothing behind its bins


def test_arithmetic_forms():
    """translation_frame 2.0: extents 4.0 (a power of two); 1.5 and 3.34: not; thres_dist 1e17 at 2e18: extents beyond 1e18 (no hoisted
    quotient, no 24-bit index); 13.36: 269 x 269 x 3 counters do not fit 64 KiB of LDS beside the tile"""
    def extent(tf, th):
        e = np.arange(-tf, tf + th - 1e-8, th).astype(F)
        return F(e[-1] - e[0]), len(e)
    r, n = extent(2.0, 0.1)
    assert (r.view(np.uint32) & 0x007fffff) == 0 and n == 41
    r, n = extent(1.5, 0.1)
    assert (r.view(np.uint32) & 0x007fffff) != 0 and 16384 + 4 * (n * n * 3 + n * 3 + 3 + 1) <= 65536    # general quotient, LDS counters
    r, n = extent(3.34, 0.1)
    assert (r.view(np.uint32) & 0x007fffff) != 0 and 16384 + 4 * n * n * 3 > 65536                       # ... global counters
    r, n = extent(2e18, 1e17)
    assert r > 1e18 and n == 41
    r, n = extent(13.36, 0.1)
    assert 16384 + 4 * n * n * 3 > 65536


def test_wide_pair_is_wide():
    s, d = vc.wide_pair(1500, 1)
    both = np.concatenate([s, d])
    ext = both.max(0) - both.min(0)
    assert 8.0 < max(ext[0], ext[1]) < 1000.0 and ext[2] < 250 * 0.2


def test_hist_batch_flags_in_between():
    X, Y = vc.hist_batch()
    for b, n in enumerate(vc.HIST_ROWS):
        for A in (X, Y):
            f = A[b, :, 3] > 0
            assert int(f.sum()) == n
            assert n == 1 or not f[np.flatnonzero(f)[0]:np.flatnonzero(f)[-1] + 1].all()   # unflagged rows between flagged ones
            assert np.abs(A[b, :, :3]).max() < 2.0                                          # ... with coordinates that would vote

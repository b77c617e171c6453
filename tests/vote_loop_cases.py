"""The inputs of tests/test_gpu_vote_loop.py (NumPy only) and the CPU restatement of what they were built for, so that
tests/test_vote_loop_cases.py can check without a GPU that every case sits on the seam of the vote's loop its name claims.

The loop (hist.hip vote_range) walks the targets [r0, r1) of a wave's z window four at a time: a ring of four reads in flight, trips
of four while eight targets or more are left, then the rest (fewer than eight) on its own.  What a wave gets is decided by
  * the window of its 64 sorted rows, restated here: wlo = zlo - max_z - slack, whi = zhi - min_z + slack,
    r0 = #(keys < wlo), r1 = #(keys <= whi) over the sorted targets of a tile (wave_windows / tile_windows);
  * the share of the window it takes when several waves share 64 rows: [r0 + len s / SPLIT, r0 + len (s + 1) / SPLIT) (shares).
Clouds are [N, 4] float32 in the pad_segment layout: valid rows first (w = 1), pads (1e8, 1e8, 1e8, 0) behind them.  The vote takes the
dst cloud as its rows (X) and the src cloud as its targets (Y); hist_icp exchanges the two where src has more valid rows (roles)."""
import numpy as np

F = np.float32
PAD = np.array([1e8, 1e8, 1e8, 0.0], F)
WAVE, TILE, SPAN = 64, 1024, 2048        # rows per wave, targets per LDS tile, targets per workgroup at most (kVoteTile, kVoteSpan)


def cloud(points, N):
    out = np.tile(PAD, (N, 1))
    p = np.asarray(points, F).reshape(-1, 3)
    assert len(p) <= N
    out[:len(p), :3] = p
    out[:len(p), 3] = 1.0
    return out


def batch(pairs, N):
    """pairs: (src points [ns, 3], dst points [nd, 3]) -> S, D [B, N, 4]"""
    return np.stack([cloud(s, N) for s, _ in pairs]), np.stack([cloud(d, N) for _, d in pairs])


def valid(c):
    return c[c[:, 3] > 0, :3]


def roles(S, D, entry):
    """Per pair (rows X, targets Y), valid points only, as the vote of `entry` takes them."""
    out = []
    for s, d in zip(S, D):
        s, d = valid(s), valid(d)
        if entry == "hist_icp" and len(s) > len(d):          # utils_match.py:139-146: src is the smaller cloud
            s, d = d, s
        out.append((d, s))
    return out


# ------------------------------------------------------------------------------------------------ the kernel's window, restated
def z_box(thres_dist=0.1):
    """(min_z, max_z) of the vote box: the first and last of the three left bin edges, float32 arange(-th, 2 th - 1e-8, th)"""
    ez = np.arange(-thres_dist, 2 * thres_dist - 1e-8, thres_dist).astype(F)
    assert len(ez) == 3
    return ez[0], ez[-1]


def wave_windows(rows, targets, min_z, max_z):
    """[(r0, r1)] per wave of 64 z-sorted rows, on the z-sorted targets: the kernel's arithmetic in float32, operation by operation"""
    zr, zt = np.sort(rows[:, 2].astype(F)), np.sort(targets[:, 2].astype(F))
    out = []
    for w in range(0, len(zr), WAVE):
        zlo, zhi = zr[w], zr[min(w + WAVE, len(zr)) - 1]
        slack = F(F(F(1e-3) * F(abs(max_z) + abs(min_z))) + F(F(1e-5) * F(abs(zlo) + abs(zhi)))) + F(1e-6)
        wlo, whi = F(F(zlo - max_z) - slack), F(F(zhi - min_z) + slack)
        out.append((int(np.searchsorted(zt, wlo, "left")), int(np.searchsorted(zt, whi, "right"))))
    return out


def tile_windows(r0, r1, ny, tile=TILE):
    """the window cut by the tiles of `tile` targets: [(r0, r1)] relative to each tile's first row"""
    return [(min(max(r0 - j0, 0), min(tile, ny - j0)), min(max(r1 - j0, 0), min(tile, ny - j0))) for j0 in range(0, ny, tile)]


def shares(r0, r1, split):
    n = max(r1 - r0, 0)
    return [(r0 + n * s // split, r0 + n * (s + 1) // split) for s in range(split)]


def trips(n):
    """(trips of four with a full trip behind them, targets of the rest) of a range of n targets"""
    k = 0
    while k + 8 <= n:
        k += 4
    return k // 4, n - k


# ------------------------------------------------------------------------------------------------ window lengths
# k targets inside the window of ONE wave of 64 rows at one height; three targets far below it (r0 = 3) and three far above.
# 0 .. 13: every residue mod 4, the empty window, one target, two trips + rest (13) when a wave takes the whole window;
# the long ones: the same for waves that take a half or a quarter of it (53 -> quarters of 13, 13, 13, 14).
WINDOW_KS = list(range(14)) + [21, 26, 27, 32, 35, 41, 47, 53]
N_BELOW = N_ABOVE = 3


def window_pair(k, seed, scale=1.0, z0=0.5):
    """(src = the targets, dst = the 64 rows).  Fewer targets than rows: no entry point exchanges the roles."""
    r = np.random.default_rng(7000 + seed)
    def pts(n, z):
        return np.c_[r.uniform(-0.5, 0.5, (n, 2)), z]
    rows = pts(WAVE, np.full(WAVE, z0))
    tg = np.concatenate([pts(N_BELOW, z0 - 5.0 + r.uniform(-0.1, 0.1, N_BELOW)), pts(k, z0 + r.uniform(-0.05, 0.05, k)),
                         pts(N_ABOVE, z0 + 5.0 + r.uniform(-0.1, 0.1, N_ABOVE))])
    r.shuffle(tg)
    assert len(tg) < WAVE
    return (tg * scale).astype(F), (rows * scale).astype(F)


def window_batch(B, N, scale=1.0):
    """pair b has WINDOW_KS[b % len] targets inside its window"""
    return batch([window_pair(WINDOW_KS[b % len(WINDOW_KS)], b, scale) for b in range(B)], N)


# ------------------------------------------------------------------------------------------------ tile seams
SEAM_NY = [1023, 1024, 1025, 2049]
SEAM_N = 2112


def seam_pair(ny, seed):
    """ny targets and ny + 7 rows (the larger cloud is the rows' under either entry point), both spread evenly over 3 m of height:
    the windows of the 64-row waves slide over every target index, the tile seams at 1024 and 2048 among them"""
    r = np.random.default_rng(8000 + seed)
    def pts(n):
        return np.c_[r.uniform(-0.5, 0.5, (n, 2)), r.uniform(0.0, 3.0, n)].astype(F)
    return pts(ny), pts(ny + 7)


def seam_batch():
    return batch([seam_pair(ny, i) for i, ny in enumerate(SEAM_NY)], SEAM_N)


# ------------------------------------------------------------------------------------------------ the box's upper face
def face_batch(tf, thres_dist=0.1):
    """Five pairs of 300 rows; in pairs 1, 2 and 4 (the last) four differences dst - src lie one float below the box's upper x face
    (and y face, pair 2): their quotient rounds to 1.0 and the bin index runs past the pair's bins -- into the next pair's, or,
    for the last pair, past the allocation (dropped)."""
    r = np.random.default_rng(77)
    hi = np.nextafter(F(np.arange(-tf, tf + thres_dist - 1e-8, thres_dist).astype(F)[-1]), F(0.0))
    pairs = []
    for b in range(5):
        s = np.c_[r.uniform(-0.6, 0.6, (300, 2)), r.uniform(0.0, 1.0, 300)].astype(F)
        d = (s + r.normal(0, 0.02, s.shape) + np.array([0.3, -0.2, 0.0])).astype(F)
        r.shuffle(d)
        if b in (1, 2, 4):
            d[:4] = (0.0, 0.0, 0.5)
            s[0] = (-hi, -hi if b == 2 else F(0.7), 0.5)
        pairs.append((s, d))
    return batch(pairs, 300), hi


# ------------------------------------------------------------------------------------------------ a wide pair
def wide_pair(n, seed):
    """A wall 24 m long (beyond the 8 m from which the vote sorts by the composite key: slabs of z, u inside a slab), and the same wall
    0.7 m further along, sampled anew"""
    r = np.random.default_rng(9000 + seed)
    def wall(m):
        return np.c_[r.uniform(0, 24.0, m), r.uniform(0, 0.4, m), r.uniform(0, 2.6, m)] + np.array([12.0, -30.0, 0.2])
    return wall(n).astype(F), (wall(n) + np.array([0.7, 0.05, 0.0])).astype(F)


# ------------------------------------------------------------------------------------------------ the drop-in hist
HIST_ROWS = [1, 3, 4, 5, 257]


def hist_batch(seed=0):
    """One pair per row count: n flagged rows in each cloud with unflagged rows IN BETWEEN (the drop-in takes flags anywhere), padded
    to 300 rows -- one tile of 1, 3, 4, 5 and 257 + gaps targets, all of them walked (no z window there)"""
    r = np.random.default_rng(9500 + seed)
    N = 300
    X, Y = np.tile(PAD, (len(HIST_ROWS), N, 1)), np.tile(PAD, (len(HIST_ROWS), N, 1))
    for b, n in enumerate(HIST_ROWS):
        for A, shift in ((X, 0.25), (Y, 0.0)):
            at = np.sort(r.choice(N, n, replace=False))
            A[b, :, :3] = r.uniform(-0.8, 0.8, (N, 3))       # unflagged rows hold ordinary coordinates: only the flag keeps them out
            A[b, :, 2] *= 0.01
            A[b, :, 3] = 0.0
            A[b, at, 3] = 1.0
            A[b, :, 0] += shift
    return X.astype(F), Y.astype(F)

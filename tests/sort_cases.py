"""The inputs of tests/test_gpu_sorts.py (NumPy only), so that tests/test_sort_restatement.py can check on the CPU that every case
is the case its name claims: ragged batches [B, N, 4] float32 in the pad_segment layout (valid rows first, w = 1; pads
(1e8, 1e8, 1e8, 0) behind them), B <= 8, N <= 8200.  No case uses a shape of the benchmark."""
import numpy as np

F = np.float32
PAD = np.array([1e8, 1e8, 1e8, 0.0], F)


def cloud(points, N):
    out = np.tile(PAD, (N, 1))
    p = np.asarray(points, F).reshape(-1, 3)
    out[:len(p), :3] = p
    out[:len(p), 3] = 1.0
    return out


def batch(pairs, N):
    """pairs: (src points [ns, 3], dst points [nd, 3]) -> S, D [B, N, 4]"""
    return np.stack([cloud(s, N) for s, _ in pairs]), np.stack([cloud(d, N) for _, d in pairs])


def shell(rng, n, centre=None, ext=None):
    """n points on three faces of a vehicle-sized box somewhere within +-40 m (the shape of synthetic._shell_points)"""
    ext = np.array([rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.0)]) if ext is None else np.asarray(ext, float)
    centre = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(0, 1.5)]) if centre is None else np.asarray(centre, float)
    face = rng.integers(0, 3, n)
    u = rng.uniform(-0.5, 0.5, (n, 3)) * ext
    for k in range(3):
        u[face == k, k] = 0.5 * ext[k]
    return (u + centre).astype(F)


# ------------------------------------------------------------------------------------------------ seams
SINGLE_COUNTS = [0, 1, 2, 63, 64, 65, 127, 129, 511, 513, 1023, 1024]      # ... and N
CHUNKED_COUNTS = [0, 1, 65, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145]


def seam_counts(N):
    """(ns, nd) of the eight pairs of a seam batch: every listed count that fits N and N itself; an empty cloud on either side, two
    pairs with swapped roles (src strictly longer), two with equal lengths"""
    if N <= 4096:
        return [(0, 1024), (1023, 0), (1, 2), (65, 63), (64, 64), (127, 129), (513, 511), (N, N)]
    if N < 6145:
        return [(0, 4097), (min(N, 4097), 0), (1, 65), (2049, 2047), (2048, 2048), (4095, 4096), (4096, 4095), (N, N)]
    return [(0, 4097), (6145, 0), (1, 65), (2049, 2047), (2048, 2048), (4095, 4096), (6144, 6143), (N, N)]


def seam_batch(N, seed=0):
    rng = np.random.default_rng(1000 + N + seed)
    pairs = []
    for ns, nd in seam_counts(N):
        c = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), 0.8])
        ext = [rng.uniform(2, 5), rng.uniform(1.2, 2.2), rng.uniform(1, 2)]
        pairs.append((shell(rng, ns, c, ext), shell(rng, nd, c + [0.3, -0.2, 0.0], ext)))
    return batch(pairs, N)


def rebatch(S, D, N):
    """the valid rows of a batch in a batch N wide"""
    out = []
    for s, d in zip(S, D):
        out.append((s[s[:, 3] > 0, :3], d[d[:, 3] > 0, :3]))
    return batch(out, N)


# ------------------------------------------------------------------------------------------------ key choice
def thin_box(n, turn_deg, seed=0, centre=(10.0, -20.0, 0.8), ext=(6.0, 0.02, 0.3)):
    """n points in a thin box, its long side turned by turn_deg about z: evenly spaced along the long side (in shuffled row order),
    so that the populations of the key bins -- and with them the margins of the key choice -- do not depend on a draw; 2 cm
    across, because what the box measures across lengthens its shadow on the directions beside its own and closes the gap
    between the best two scores"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(ext)
    u[:, 0] = ((rng.permutation(n) + 0.5) / n - 0.5) * ext[0]
    a = np.deg2rad(turn_deg)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return (u @ R.T + np.asarray(centre)).astype(F)


def cube(n, seed=0, lo=(-3.0, 5.0, 0.0), edge=2.0):
    """n points in a cube whose three extents are EXACTLY equal (opposite corners are rows 0 and 1) -> code 0"""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(0, 1, (n, 3)) * edge + np.asarray(lo)).astype(F)
    p[0] = np.asarray(lo, F)
    p[1] = np.asarray(lo, F) + F(edge)
    return p


def box_e1_eq_e2(n, seed=0):
    """extents (1, 2, 2) exactly: e1 = e2 > e0 -> code 1"""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(0, 1, (n, 3)) * [1.0, 2.0, 2.0] + [4.0, 8.0, 0.0]).astype(F)
    p[0] = (4.0, 8.0, 0.0)
    p[1] = (5.0, 10.0, 2.0)
    return p


def key_choice_batch(N):
    """The hand-made clouds as FIXED clouds at the thresholds of the direction keys (ny = 1024 / 1025, nx = 511 / 512).
    -> S, D, names, want; want[b]: 'direction' (code 4 chosen), 'legacy' (a direction was allowed and the longest axis kept),
    'below' (no direction allowed: a threshold not reached)"""
    t45 = lambda n, s: thin_box(n, 45.0, seed=s)       # noqa: E731
    t0 = lambda n, s: thin_box(n, 0.0, seed=s)         # noqa: E731
    big = min(N, 2000)
    spec = [("turned_1025_vs_512", t45(512, 1), t45(1025, 2), "direction"),
            ("turned_1024_vs_512", t45(512, 3), t45(1024, 4), "below"),
            ("turned_1025_vs_511", t45(511, 5), t45(1025, 6), "below"),
            ("turned_big", t45(big - 1, 7), t45(big, 8), "direction"),
            ("aligned_big", t0(big - 1, 9), t0(big, 10), "legacy"),
            ("cube_1025_vs_600", cube(600, 11), cube(1025, 12), "legacy"),
            ("e1_eq_e2_1025_vs_600", box_e1_eq_e2(600, 13), box_e1_eq_e2(1025, 14), "legacy"),
            ("turned_swapped", t45(1100, 15), t45(700, 16), "direction")]     # (the src cloud is the longer one: it is the fixed role)
    S, D = batch([(s, d) for _, s, d, _ in spec], N)
    return S, D, [n for n, _, _, _ in spec], [w for _, _, _, w in spec]


# ------------------------------------------------------------------------------------------------ ties
def ties_batch(N):
    """-> S, D, names, ties; ties[b]: the least number of rows of the dst cloud that share a key with another row, under the axis
    key AND under z (the CPU test counts them).  Every pair is sorted along x (the extents say so) and has equal z ties as well,
    because each cloud is a set of (x, y, z) with x and z drawn from the same few values."""
    rng = np.random.default_rng(77)
    n = min(N, 6000)

    def lattice(vals, n, yspread=1e-3):
        """x and z from `vals` (x's extent the largest), y anything narrower"""
        v = np.asarray(vals, F)
        p = np.empty((n, 3), F)
        p[:, 0] = v[rng.integers(0, len(v), n)]
        p[:, 1] = rng.uniform(0, yspread, n).astype(F)
        p[:, 2] = (v[rng.integers(0, len(v), n)] * F(0.25)).astype(F)
        p[0, 0], p[1, 0] = v.min(), v.max()
        return p

    den = np.array([1e-45, -1e-45, 3e-45, -3e-45, 1e-40, -1e-40, 0.0], F)      # denormal keys on both sides of zero
    zero = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], F)
    three = lattice([-1.0, 0.0, 1.5], n)
    spec = [("three_keys", three, lattice([-1.0, 0.0, 1.5], n), n - 3),
            ("one_key", lattice([2.5], n, 0.0), lattice([2.5], n - 1, 0.0), n - 1),
            ("duplicates", np.repeat(shell(rng, n // 2, ext=(5, 1, 1)), 2, axis=0), np.repeat(shell(rng, (n - 2) // 2, ext=(5, 1, 1)), 2, axis=0), n - 2),
            ("signed_zeros", lattice(zero, n), lattice(zero, n - 5), n - 5 - 6),
            ("denormals", lattice(den, n, 0.0), lattice(den, n - 7, 0.0), n - 7 - 7),
            ("near_3000", lattice([2999.9998, 3000.0, 3000.0002, -3000.0, -2999.9998], n), lattice([2999.9998, 3000.0, 3000.0002, -3000.0, -2999.9998], n - 9), n - 9 - 5),
            ("near_1e6", lattice([999999.94, 1e6, 1000000.06, -1e6, -999999.94], n), lattice([999999.94, 1e6, 1000000.06, -1e6, -999999.94], n - 11), n - 11 - 5)]
    S, D = batch([(s, d) for _, s, d, _ in spec], N)
    return S, D, [n_ for n_, _, _, _ in spec], [t for _, _, _, t in spec]


# ------------------------------------------------------------------------------------------------ the wide vote key
WIDE_EZ = np.array([-0.125, 0.0, 0.125], F)      # h = 0.25 exactly


def wall(n, seed, axis=0, length=40.0, height=3.0, z_range=None, slab_rows=0, origin=(-20.0, 3.0, 0.0)):
    """n points on a wall `length` m along `axis`, `height` m high (or z over z_range); the first rows are the corners of its
    box, and `slab_rows` rows have z = z0 + k * 0.25 exactly (on a slab border for h = 0.25)"""
    rng = np.random.default_rng(seed)
    zr = height if z_range is None else z_range
    p = np.empty((n, 3))
    p[:, axis] = rng.uniform(0, length, n)
    p[:, 1 - axis] = rng.uniform(0, 0.2, n)
    p[:, 2] = rng.uniform(0, zr, n)
    p[0] = 0.0
    p[1, axis], p[1, 1 - axis], p[1, 2] = length, 0.2, zr
    if slab_rows:
        p[2:2 + slab_rows, 2] = 0.25 * rng.integers(0, int(zr / 0.25) + 1, slab_rows)
    o = np.asarray(origin, float)
    if axis == 1:
        o = o[[1, 0, 2]]
    return (p + o).astype(F)


def wide_batch(N):
    """-> S, D, names, want; want[b] = (wide, uaxis)"""
    spec = [("wall_x_4097_rows", wall(2049, 1, slab_rows=400), wall(2048, 2, slab_rows=400), (1, 0)),
            ("wall_x_4096_rows", wall(2048, 3), wall(2048, 4), (0, 0)),
            ("wall_y", wall(2500, 5, axis=1, slab_rows=300), wall(2100, 6, axis=1), (1, 1)),
            ("extent_just_under_8", wall(2300, 7, length=7.999999), wall(2300, 8, length=7.999999), (0, 0)),
            ("extent_just_over_8", wall(2300, 9, length=8.000001), wall(2300, 10, length=8.000001), (1, 0)),
            ("z_range_250_h", wall(2300, 11, z_range=62.5), wall(2300, 12, z_range=62.5), (0, 0)),
            ("z_range_below_250_h", wall(min(N, 4500), 13, z_range=62.25, slab_rows=500), wall(2300, 14, z_range=62.25), (1, 0))]
    S, D = batch([(s, d) for _, s, d, _ in spec], N)
    return S, D, [n for n, _, _, _ in spec], [w for _, _, _, w in spec]

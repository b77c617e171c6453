"""Hand-built inputs for icpflow_ground_segment on its own (tests/test_ground_cases.py proves on the CPU that each is the case its
name claims, tests/test_gpu_ground_cases.py runs each through the C ABI): points placed patch by patch like
ground_scenes.in_patch, but from the case's OWN Params.  A case is dict(pts float32 [n, 3], params, claim, ...) and belongs to
a group:

  P  parameters   one parameter away from its default; the scene is built so that the default value gives another result
  S  strides      the mixed scene of P at the default parameters (the forms are the GPU test's)
  N  sort         all-ground scenes at the sizes where carve() changes, and the compositions of a tile of 64 rows
  L  seeds        ties among the lowest heights, lows at late places, exactly num_lpr candidates, one fewer after the skip
  R  revert       a flatness list of 95 values, 32 candidates in one ring, 1500 and 1501 ground points
  E  plane solve  patches on exact lattices (the moments are exact in fp64), with two named degenerate patches beside them

carve(n) restates csrc/ground.hip's carve: the binning waves and the rows of each.  Not a test module."""
import functools

import numpy as np

import ground_restatement as gr

F = np.float32
CHUNK_MIN, MAX_WAVES, WAVE = 512, 1024, 64
N_SIZES = (10, 63, 64, 65, 511, 512, 513, 1024, 1025, 4608, 4609, 524288, 524289, 600000)
N_LARGE = (524288, 524289, 600000)


def carve(n):
    """(waves, chunk): wave w bins the rows [w * chunk, min((w + 1) * chunk, n))"""
    waves = min(max(-(-n // CHUNK_MIN), 1), MAX_WAVES)
    per = -(-n // waves)
    return waves, -(-per // WAVE) * WAVE


def patch_zrs(p):
    """(zone, ring, sector) of patch ids, arrays allowed"""
    p = np.asarray(p)
    zone = np.searchsorted(np.asarray(gr.PATCH_BASE), p, side="right") - 1
    q = p - np.asarray(gr.PATCH_BASE)[zone]
    return zone, q // np.asarray(gr.SECTORS)[zone], q % np.asarray(gr.SECTORS)[zone]


def in_patch(rng, par, zone, ring, sector, m=None, r_span=(0.06, 0.94), t_span=(0.06, 0.94)):
    """points (x, y) inside a patch of `par`'s zone model, away from its borders; zone, ring, sector may be arrays (m = None)"""
    zone, ring, sector = np.asarray(zone), np.asarray(ring), np.asarray(sector)
    lo, rs, ss = np.asarray(par.lo)[zone], np.asarray(par.ring_size)[zone], np.asarray(gr.SECTOR_SIZE)[zone]
    size = zone.shape if m is None else m
    r = lo + rs * (ring + rng.uniform(r_span[0], r_span[1], size))
    t = ss * (sector + rng.uniform(t_span[0], t_span[1], size))
    return r * np.cos(t), r * np.sin(t)


def flat(rng, par, zone, ring, sector, m, z, sigma=0.01, **kw):
    x, y = in_patch(rng, par, zone, ring, sector, m, **kw)
    return np.stack([x, y, z + sigma * rng.standard_normal(m)], axis=1)


def ramp(rng, par, zone, ring, sector, m, slope, z_mid, sigma=0.01, noise="normal", **kw):
    """a plane rising outwards: z = z_mid + slope * (r - r_mid)"""
    x, y = in_patch(rng, par, zone, ring, sector, m, **kw)
    r0, r1, _, _ = gr.patch_bounds(zone, ring, sector, par)
    e = sigma * rng.standard_normal(m) if noise == "normal" else rng.uniform(-sigma, sigma, m)
    return np.stack([x, y, z_mid + slope * (np.hypot(x, y) - 0.5 * (r0 + r1)) + e], axis=1)


def bowl(rng, par, zone, ring, sector, m, z0, rise, sigma=0.003):
    """a surface that curves upwards outwards: z = z0 + rise * u^2, u from 0 to 1 across the ring"""
    x, y = in_patch(rng, par, zone, ring, sector, m)
    r0, r1, _, _ = gr.patch_bounds(zone, ring, sector, par)
    u = (np.hypot(x, y) - r0) / (r1 - r0)
    return np.stack([x, y, z0 + rise * u * u + sigma * rng.standard_normal(m)], axis=1)


def wall(rng, par, zone, ring, sector, m, z_lo, z_hi, at=0.5, sigma=0.003):
    """a thin vertical sheet, 0.8 m long, along a ray of the patch (`at` of its angle): short, so that the lowest slice of it, a
    few centimetres high, is still a plane and not a line ((s1 - s2) / s0 stays over 1e-3)"""
    r0, r1, t0, t1 = gr.patch_bounds(zone, ring, sector, par)
    r = 0.5 * (r0 + r1) + rng.uniform(-0.4, 0.4, m)
    t = t0 + at * (t1 - t0)
    off = sigma * rng.standard_normal(m)
    return np.stack([r * np.cos(t) - off * np.sin(t), r * np.sin(t) + off * np.cos(t), rng.uniform(z_lo, z_hi, m)], axis=1)


def _finish(rng, parts, shuffle=True):
    pts = np.concatenate(list(parts.values())).astype(F)
    names = np.concatenate([np.full(len(v), k) for k, v in enumerate(parts.values())])
    if shuffle:
        perm = rng.permutation(len(pts))
        pts, names = pts[perm], names[perm]
    return pts, {k: np.flatnonzero(names == j) for j, k in enumerate(parts)}


# ---- P: the mixed scene ---------------------------------------------------------------------------------------------------
def mixed(par, seed=21):
    """One scene with something for every parameter to decide, built from `par`'s ranges and sensor height; g = the ground's
    height, 0.07 above -sensor_height.  What each part is for stands beside it."""
    rng = np.random.default_rng(seed)
    g = -par.sensor_height + 0.07
    deg = lambda a: np.tan(np.radians(a))   # noqa: E731
    plain = [flat(rng, par, 0, 0, s, 30, g) for s in (0, 12, 15)] + [flat(rng, par, 0, 1, s, 30, g) for s in (0, 4, 8, 12)]
    plain += [flat(rng, par, 1, r, s, 30, g) for r in range(4) for s in (0, 10, 20)] + [flat(rng, par, 2, 1, s, 30, g) for s in (0, 20, 40)]
    plain += [flat(rng, par, 3, r, s, 30, g) for r in (0, 3) for s in (5, 25)]
    parts = dict(plain=np.concatenate(plain))
    # num_min_pts: patches of 12, 29 and 30 rows (ground at 10, the first two not at 30); of one row each (a NaN plane at 1)
    parts["twelve"] = np.concatenate([flat(rng, par, 3, 2, s, 12, g) for s in (3, 5)])
    parts["twentynine"] = flat(rng, par, 3, 2, 11, 29, g)
    parts["thirty"] = flat(rng, par, 3, 2, 13, 30, g)
    parts["single"] = np.concatenate([flat(rng, par, 2, 3, s, 1, g) for s in range(1, 49, 2)])
    # th_dist: a kerb 0.08 and a step 0.2 above the ground
    parts["kerb"] = np.concatenate([flat(rng, par, 1, 1, 3, 100, g), flat(rng, par, 1, 1, 3, 40, g + 0.08), flat(rng, par, 1, 1, 3, 40, g + 0.2)])
    # num_lpr 1 / 5 and th_seeds 0.05: six rows 0.3 below the ground (the seeds are they alone, or they and the ground)
    parts["pit"] = np.concatenate([flat(rng, par, 1, 2, 6, 80, g), flat(rng, par, 1, 2, 6, 6, g - 0.3)])
    # num_lpr 64 and th_seeds 0.5: one row 6.3 below (the only seed, a NaN plane, unless the mean or the threshold rises)
    parts["outlier"] = np.concatenate([flat(rng, par, 1, 2, 12, 80, g), flat(rng, par, 1, 2, 12, 1, g - 6.3)])
    # th_seeds_v (0.05 / 0.2 / 0.25) and th_dist_v: walls that reach 0.15, 0.24 and 0.35 below the ground, zone 0 and zone 1
    for k, (depth, s0, s1) in enumerate(((0.15, 1, 4), (0.24, 2, 5), (0.35, 5, 6))):
        parts[f"wall0_{k}"] = np.concatenate([flat(rng, par, 0, 0, s0, 400, g, sigma=0.004), wall(rng, par, 0, 0, s0, 400, g - depth, g + 0.5)])
        parts[f"wall1_{k}"] = np.concatenate([flat(rng, par, 1, 1, s1, 400, g, sigma=0.004), wall(rng, par, 1, 1, s1, 400, g - depth, g + 0.5)])
    # num_iter in R-VPF: three walls of one patch, each the lowest once the one before is gone (the floor is 0.65 above g)
    parts["walls3"] = np.concatenate([flat(rng, par, 0, 1, 5, 200, g + 0.65), wall(rng, par, 0, 1, 5, 300, g - 0.4, g + 1.2, at=0.25),
                                      wall(rng, par, 0, 1, 5, 300, g - 0.1, g + 1.2, at=0.5), wall(rng, par, 0, 1, 5, 300, g + 0.2, g + 1.2, at=0.75)])
    # num_iter in R-GPF (and final_plane): surfaces that curve upwards; every refit reaches further up
    parts["bowl2"] = bowl(rng, par, 2, 0, 8, 600, g, 1.6)
    parts["bowl3"] = bowl(rng, par, 3, 1, 9, 600, g, 2.4)
    # uprightness_thr 0.5 / 0.707 / 0.9: normals at 20, 35, 52 and 65 degrees from the vertical, near (falling) and far (rising);
    # narrow ones, so that the lowest slice of a steep one is still a plane and a near one stays above the zone-0 skip
    for a, s, t in ((20, 6, 22), (35, 9, 28), (52, 10, 34), (65, 13, 37)):
        parts[f"near{a}"] = ramp(rng, par, 0, 1, s, 200, -deg(a), g + 0.6, sigma=0.002, r_span=(0.42, 0.58), t_span=(0.45, 0.55))
        parts[f"far{a}"] = ramp(rng, par, 2, 2, t, 200, deg(a), g + 0.7, sigma=0.002, t_span=(0.4, 0.6))
    # adaptive_seed_selection_margin x sensor_height: rows 0.25 below the ground (under -1.0 h only), 0.6 below (under -1.0 h and
    # -1.2 h, over -2.0 h), 2.0 below (under all of them); patches of such rows only; one with 60 of its 100 rows below (fewer candidates than num_lpr = 64)
    parts["below_a"] = np.concatenate([flat(rng, par, 0, 1, 1, 150, g), flat(rng, par, 0, 1, 1, 15, g - 0.25)])
    parts["below_b"] = np.concatenate([flat(rng, par, 0, 1, 2, 150, g), flat(rng, par, 0, 1, 2, 15, g - 0.6)])
    parts["deep"] = np.concatenate([flat(rng, par, 0, 0, 6, 120, g - 2.0), flat(rng, par, 0, 0, 9, 150, g), flat(rng, par, 0, 0, 9, 15, g - 2.0)])
    parts["all_below"] = flat(rng, par, 0, 0, 13, 120, g - 0.8)
    parts["most_below"] = np.concatenate([flat(rng, par, 0, 0, 14, 40, g), flat(rng, par, 0, 0, 14, 60, g - 0.8)])
    # boxes on the ground
    parts["boxes"] = np.concatenate([np.concatenate([flat(rng, par, z, r, s, 40, g), in_box(rng, par, z, r, s, 60, g)])
                                     for z, r, s in ((0, 0, 10), (1, 0, 5), (2, 1, 6))])
    return parts


def in_box(rng, par, zone, ring, sector, m, g):
    x, y = in_patch(rng, par, zone, ring, sector, m, r_span=(0.4, 0.6), t_span=(0.4, 0.6))
    return np.stack([x, y, rng.uniform(g, g + 2.0, m)], axis=1)


def _border_rows(par, g, steps):
    """rows on the four axes at r = every ring border of `par` (steps False: ON it, for radii exact in float32) or one float32
    step below and above min_range, max_range and every zone edge (steps True)"""
    if steps:
        radii = []
        for e in (par.min_range, par.max_range) + par.lo[1:]:
            a = F(e)
            below, above = (a, np.nextafter(a, F(np.inf))) if np.float64(a) < e else (np.nextafter(a, F(-np.inf)), a)
            radii += [below, above] if np.float64(above) > e else [below, above, np.nextafter(above, F(np.inf))]
    else:
        radii = [F(par.lo[k] + j * par.ring_size[k]) for k in range(4) for j in range(gr.RINGS[k])] + [F(par.max_range)]
    rows = []
    for r in radii:
        rows += [[r, 0.0, g], [0.0, r, g], [-r, 0.0, g], [0.0, -r, g]]
    return np.asarray(rows, dtype=np.float64)


def _with_borders(par, seed, steps):
    """the mixed scene + the border rows + 30 ground rows in every patch a border row falls into (a patch of rows on either side
    of each border: the axes' patches of every ring)"""
    rng = np.random.default_rng(seed + 1)
    g = -par.sensor_height + 0.07
    parts = mixed(par, seed)
    special = _border_rows(par, g, steps)
    parts["special"] = special
    axes = []
    for zone in range(4):
        S = gr.SECTORS[zone]
        for ring in range(gr.RINGS[zone]):
            for sector in sorted({S - 1, 0, S // 4 - 1, S // 4, S // 2 - 1, S // 2, (3 * S) // 4 - 1, (3 * S) // 4}):
                axes.append(flat(rng, par, zone, ring, sector, 30, g))
    parts["axes"] = np.concatenate(axes)
    return rng, parts


P_VALUES = dict(num_iter=(1, 2, 5), num_lpr=(1, 5, 64), num_min_pts=(1, 30), th_dist=(0.05, 0.3), th_seeds=(0.05, 0.5),
                th_seeds_v=(0.05, 0.2), th_dist_v=(0.05, 0.2), uprightness_thr=(0.5, 0.9), adaptive_seed_selection_margin=(-1.0, -2.0, 0.0))


def _p_cases():
    out = {}
    for field, values in P_VALUES.items():
        for v in values:
            out[f"{field}[{v}]"] = functools.partial(_p_case, field, v)
    out["ranges_dyadic"] = functools.partial(_p_ranges, gr.DEFAULT.replace(min_range=2.0, max_range=66.0), False)
    out["ranges_2p7_80"] = functools.partial(_p_ranges, gr.DEFAULT.replace(min_range=2.7, max_range=80.0, sensor_height=1.9), True)
    return out


def _p_case(field, v):
    par = gr.DEFAULT.replace(**{field: v})
    rng = np.random.default_rng(22)
    pts, parts = _finish(rng, mixed(par))
    return dict(pts=pts, parts=parts, params=par, default=gr.DEFAULT, claim=f"the mixed scene judged with {field} = {v}: another result than at the default")


def _p_ranges(par, steps):
    rng, parts = _with_borders(par, 23, steps)
    pts, parts = _finish(rng, parts)
    what = "one float32 step inside and outside min_range, max_range and every zone edge" if steps else "ON every ring and zone border"
    return dict(pts=pts, parts=parts, params=par, default=gr.DEFAULT,
                claim=f"ranges {par.min_range} .. {par.max_range}, sensor height {par.sensor_height}: rows on the four axes {what}")


# ---- S ----------------------------------------------------------------------------------------------------------------------
def _s_mixed():
    rng = np.random.default_rng(24)
    parts = mixed(gr.DEFAULT)
    parts["out"] = np.float64([[70.0, 1.0, -1.7], [0.3, 0.2, -1.7], [np.nan, 0.0, 0.0], [3.0, np.inf, 0.0]] * 5)
    pts, parts = _finish(rng, parts)
    return dict(pts=pts, parts=parts, params=gr.DEFAULT, claim="the mixed scene at the default parameters, with rows that take no part")


# ---- N: all ground ----------------------------------------------------------------------------------------------------------
G0 = -1.65


def ground_rows(rng, par, pid, sigma=0.01):
    """one ground row in the patch pid[i] for every i, in that order; -1: a row out of range (r = 70), -2: a NaN row"""
    pid = np.asarray(pid)
    inside = pid >= 0
    zone, ring, sector = patch_zrs(np.where(inside, pid, 0))
    x, y = in_patch(rng, par, zone, ring, sector)
    z = G0 + sigma * rng.standard_normal(len(pid))
    pts = np.stack([x, y, z], axis=1)
    pts[pid == -1] = (70.0, 3.0, G0)
    pts[pid == -2] = (np.nan, 1.0, G0)
    return pts.astype(F)


def _n_size(n):
    rng = np.random.default_rng(1000 + n % 997)
    k = 1 if n < 20 else 2 if n < 511 else 20 if n < 4608 else 100 if n < 100000 else gr.PATCHES
    chosen = rng.choice(gr.PATCHES, k, replace=False)
    pid = np.concatenate([chosen[np.arange(10 * k) % k], chosen[rng.integers(0, k, max(n - 10 * k, 0))]])[:n]      # at least 10 rows each
    pid = pid[rng.permutation(n)]
    return dict(pts=ground_rows(rng, gr.DEFAULT, pid), pid=pid, params=gr.DEFAULT, all_ground=True,
                claim=f"{n} ground rows in {k} patches: (waves, chunk) = {carve(n)}")


def _n_tile(kind):
    rng = np.random.default_rng(31)
    if kind == "tile_64_patches":              # 40 tiles of 64 rows, each a permutation of the same 64 patches
        chosen = rng.choice(gr.PATCHES, 64, replace=False)
        pid = np.concatenate([chosen[rng.permutation(64)] for _ in range(40)])
        claim = "every full tile of 64 rows holds 64 different patches"
    elif kind == "tile_one_patch":
        chosen = np.sort(rng.choice(gr.PATCHES, 30, replace=False))
        pid = np.sort(chosen[np.arange(3000) % 30])
        claim = "rows sorted by patch: a tile holds one patch, or two at a change"
    elif kind == "tile_two_alternating":
        pid = np.where(np.arange(3000) % 2 == 0, 7, 300)
        claim = "two patches, row by row in turn"
    elif kind == "tile_unbinned":              # 8 chunks of 512: chunk 3 and the tile at 1024 + 128 hold no binned row
        n = 4096
        chosen = rng.choice(gr.PATCHES, 12, replace=False)
        pid = np.where(np.arange(n) % 2 == 0, -1, -2)
        at = np.arange(0, n, 4) + rng.integers(0, 4, n // 4)
        pid[at] = chosen[np.arange(len(at)) % 12]
        pid[3 * 512: 4 * 512] = -1
        pid[1024 + 128: 1024 + 192] = -2
        claim = "three of four rows out of range or NaN; chunk 3 and the tile at row 1152 hold no binned row"
    else:                                      # one_patch_every_wave
        n = 40000
        chosen = rng.choice(np.arange(1, gr.PATCHES), 40, replace=False)
        pid = np.concatenate([np.zeros(20000, dtype=np.int64), chosen[np.arange(20000) % 40]])[rng.permutation(n)]
        claim = "patch 0 has 20 000 rows in every one of the 79 binning waves, other patches' rows between them"
    return dict(pts=ground_rows(rng, gr.DEFAULT, pid), pid=pid, params=gr.DEFAULT, all_ground=True, claim=claim)


# ---- L: seeds ---------------------------------------------------------------------------------------------------------------
L_PAR = gr.DEFAULT.replace(num_iter=1, th_dist=0.03)     # one round, a narrow band: the labels show the plane of the seeds


def _l_ties():
    """One patch of zone 1.  15 rows at a = -1.80 and 15 at b = -1.76 (float32 values), in the inner 60 % of the ring: the 20
    lowest are 15 + 5, the threshold is (15 a + 5 b) / 20 + 0.125.  With 19 seeds it is 1.6e-3 lower, with 21 1.4e-3 higher, and
    counting a tie once takes 18 higher rows for a and b.  12 rows stand between the 19-threshold and the right one and 12 between
    the right one and the 21-threshold, the first at the outer rim and the second at the inner one, 0.12 above the lows: a seed set with or without them is another
    plane.  200 rows rise outwards from -1.66 to -1.60 along the plane that the right seeds give."""
    rng = np.random.default_rng(41)
    par, (z, r, s) = L_PAR, (1, 0, 9)
    a, b = np.float64(F(-1.80)), np.float64(F(-1.76))
    thr = {k: (15 * a + (k - 15) * b) / k + par.th_seeds for k in (19, 20, 21)}
    x, y = in_patch(rng, par, z, r, s, 30, r_span=(0.06, 0.6))
    lows = np.stack([x, y, np.where(rng.permutation(30) < 15, a, b)], axis=1)
    x, y = in_patch(rng, par, z, r, s, 12, r_span=(0.88, 0.94))
    x2, y2 = in_patch(rng, par, z, r, s, 12, r_span=(0.06, 0.12))
    x, y = np.concatenate([x, x2]), np.concatenate([y, y2])
    between = np.stack([x, y, np.repeat([0.5 * (thr[19] + thr[20]), 0.5 * (thr[20] + thr[21])], 12)], axis=1)
    rest = ramp(rng, par, z, r, s, 200, 0.06 / par.ring_size[z], -1.62, sigma=0.004)
    pts, parts = _finish(rng, dict(lows=lows, between=between, rest=rest, plain=flat(rng, par, 1, 0, 20, 30, G0)))
    return dict(pts=pts, parts=parts, params=par, patch=gr.patch_index(z, r, s), thresholds=thr, wrong=("z_only", 19, 21),
                claim="15 + 15 tied heights: the 20 lowest are 15 + 5")


def _l_late():
    """Patches of 257, 513 and 1025 rows (zone 1, no skip).  Their 20 lowest rows, 0.3 below the rest, are their LAST 20 rows in
    row order, the lowest of all the very last: places 237 .. 256, 493 .. 512, 1005 .. 1024."""
    rng = np.random.default_rng(42)
    par, rows, pids = gr.DEFAULT, [], []
    for m, s in ((257, 2), (513, 12), (1025, 22)):
        high = flat(rng, par, 1, 1, s, m - 20, G0)
        low = flat(rng, par, 1, 1, s, 20, G0 - 0.3, sigma=0.0)
        low[:, 2] = G0 - 0.3 - 0.001 * np.arange(20)
        rows += [high, low]
        pids.append(gr.patch_index(1, 1, s))
    other = flat(rng, par, 1, 2, 3, 600, G0)
    body = np.concatenate(rows)
    # other patches' rows between them, the order inside each patch kept
    slots = np.sort(rng.choice(len(body) + len(other), len(body), replace=False))
    pts = np.empty((len(body) + len(other), 3))
    mask = np.zeros(len(pts), dtype=bool)
    mask[slots] = True
    pts[mask], pts[~mask] = body, other
    return dict(pts=pts.astype(F), params=par, patches=pids, sizes=(257, 513, 1025), wrong=(19, 21),
                claim="the 20 lowest rows of patches of 257, 513 and 1025 rows are their last 20 places")


def _l_exact():
    """`exactly_20`: a zone-1 patch of exactly 20 rows, 10 of them 0.2 below the others: every row is a seed candidate and the
    selection ends with its last key.  `19_after_skip`: a zone-0 patch of 40 rows, 21 of them below -1.2 x sensor_height: 19
    candidates, the selection runs dry one round early."""
    rng = np.random.default_rng(43)
    par = L_PAR
    twenty = np.concatenate([flat(rng, par, 1, 0, 4, 10, G0 - 0.2, r_span=(0.06, 0.5)), flat(rng, par, 1, 0, 4, 10, G0, r_span=(0.5, 0.94))])
    x, y = in_patch(rng, par, 0, 1, 4, 19)
    up = np.stack([x, y, np.linspace(G0, G0 + 0.19, 19)], axis=1)
    nineteen = np.concatenate([up, flat(rng, par, 0, 1, 4, 21, -2.5)])
    pts, parts = _finish(rng, dict(twenty=twenty, nineteen=nineteen, plain=flat(rng, par, 1, 0, 20, 30, G0)))
    return dict(pts=pts, parts=parts, params=par, patches=(gr.patch_index(1, 0, 4), gr.patch_index(0, 1, 4)), wrong=(19,),
                claim="a patch with exactly num_lpr candidates and one with num_lpr - 1 after the zone-0 skip")


def _l_final_plane():
    """the curved surfaces of the mixed scene after ONE round: the set that the seeds' plane decides and the set of the plane
    fitted to it differ"""
    rng = np.random.default_rng(44)
    par = gr.DEFAULT.replace(num_iter=1)
    parts = dict(bowl2=bowl(rng, par, 2, 0, 8, 600, G0, 1.6), bowl3=bowl(rng, par, 3, 1, 9, 600, G0, 2.4), plain=flat(rng, par, 1, 0, 20, 30, G0))
    pts, parts = _finish(rng, parts)
    return dict(pts=pts, parts=parts, params=par, claim="the last set is the one the plane BEFORE it decides, not the plane fitted to it")


# ---- R: revert --------------------------------------------------------------------------------------------------------------
def candidate(rng, par, zone, ring, sector, m, sigma, noise="normal", **kw):
    """a ramp that rises outwards through z >= 0: upright, heading < 0, elevated"""
    return ramp(rng, par, zone, ring, sector, m, 0.2, 0.3, sigma=sigma, noise=noise, **kw)


def _r_list95():
    rng = np.random.default_rng(51)
    par, parts = gr.DEFAULT, {}
    near = [(0, 0, s) for s in range(16)] + [(0, 1, s) for s in range(16)] + [(1, 0, s) for s in range(32)] + [(1, 1, s) for s in range(31)]
    # rings 0 to 2 rough, ring 3 smooth, the candidate between them: reverted by the whole list, rejected by ring 3's own values
    parts["ground"] = np.concatenate([flat(rng, par, z, r, s, 24, G0, sigma=rng.uniform(0.004, 0.006) if (z, r) == (1, 1) else rng.uniform(0.025, 0.035))
                                      for z, r, s in near])
    parts["lone"] = candidate(rng, par, 1, 1, 31, 150, 0.02)
    pts, parts = _finish(rng, parts)
    return dict(pts=pts, parts=parts, params=par, claim="ring 3's one candidate is decided against a flatness list of 95 values")


def _r_cand32():
    rng = np.random.default_rng(52)
    par, parts = gr.DEFAULT, {}
    parts["ground"] = np.concatenate([flat(rng, par, 0, r, s, 40, G0, sigma=0.02) for r in range(2) for s in range(0, 16, 2)])
    sig = np.concatenate([np.linspace(0.003, 0.012, 16), np.linspace(0.035, 0.06, 16)])[rng.permutation(32)]
    parts["ramps"] = np.concatenate([candidate(rng, par, 1, 0, s, 120, sig[s]) for s in range(32)])
    pts, parts = _finish(rng, parts)
    return dict(pts=pts, parts=parts, params=par, claim="all 32 sectors of ring 2 are candidates, reverted and rejected ones among them")


def _r_dense(m):
    """a rough candidate (uniform noise of +-0.06: every row within th_dist of its plane, flatness 1.2e-3 < th_dist^2) of exactly m
    rows next to smooth ground: by its probability it is rejected; beyond 1500 ground points it is reverted"""
    rng = np.random.default_rng(53)
    par = gr.DEFAULT
    parts = dict(ground=np.concatenate([flat(rng, par, 0, 1, s, 40, G0, sigma=0.01) for s in range(0, 8)]),
                 dense=candidate(rng, par, 0, 1, 10, m, 0.06, noise="uniform"))
    pts, parts = _finish(rng, parts)
    return dict(pts=pts, parts=parts, params=par, patch=gr.patch_index(0, 1, 10), claim=f"a candidate of exactly {m} ground points")


# ---- E: the plane solve on exact lattices ---------------------------------------------------------------------------------
def _lattice(x0, y0, nx, ny, step):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return i.ravel(), j.ravel(), x0 + i.ravel() * step, y0 + j.ravel() * step


E_PATCH = dict(flat_exact=(1, 1, 3), tilt_exact=(1, 1, 4), square_lattice=(1, 2, 3), thin_strip=(2, 1, 6), far_small=(3, 3, 3),
               collinear=(3, 2, 10), copies=(3, 2, 20))
E_DEGENERATE = ("collinear", "copies")
E_Z = np.float64(F(-1.65))


def _e_parts(rng):
    """Every coordinate but flat_exact's z is a multiple of 2^-6 below 64, so every centred product is a multiple of 2^-24 and
    every sum of them exact in fp64; the sets have 64 or 288 points, and the means of the sets of 64 are exact too.
      flat_exact      8 x 8, step 1/8, z one float32 value: the covariance is diag(v, v, 0) and no rotation is taken
      tilt_exact      8 x 8, y at -7, -3, -2, -1, 1, 2, 3, 7 sixteenths about its middle (the squares sum to 126 = 2 x 63, so the
                      variance is w = 2^-4 exactly), z = y / 4 - 1/4 (elevated, heading < 0: a revert candidate): the covariance
                      is [[v, 0, 0], [0, w, w/4], [0, w/4, w/16]], whose one rotation has theta = -15/8, sqrt(1 + theta^2) = 17/8,
                      t = -1/4, every step exact, and leaves a smallest value of EXACTLY 0 -- with flat_exact's 0 the only listed flatness, the revert computes 0 / 0
      square_lattice  8 x 8, z a checkerboard of 1/64: diag(v, v, w) exactly, s0 == s1
      thin_strip      96 x 3 on the diagonals (x = x0 + (i + 2 j) / 64, y = y0 + (i - 2 j) / 64), z a checkerboard of 1/64:
                      s1 / s0 = 3.5e-3 and (s1 - s2) / s0 = 3.3e-3 -- a strip of s1 / s0 = 1e-4 cannot keep the gap of 1e-3
                      that makes its normal defined, so this one is as thin as the gap allows with a margin of 3
      far_small       8 x 8 of 1/8 at r = 60 m, z = -106/64 + (i + 2 j + (i j) mod 3) / 64: a tilted, slightly rough plane, so that
                      every pair of axes is rotated
      collinear       30 points of one line (a single scan ring in a far patch): no plane; named, left out
      copies          10 copies of one point: no plane; named, left out"""
    parts = {}
    i, j, x, y = _lattice(8.625, 7.0, 8, 8, 0.125)
    parts["flat_exact"] = np.stack([x, y, np.full(64, E_Z)], axis=1)
    i, j, x, y = _lattice(7.0, 8.625, 8, 8, 0.125)
    y = 9.0625 + np.asarray([-7, -3, -2, -1, 1, 2, 3, 7])[j] / 16
    parts["tilt_exact"] = np.stack([x, y, y / 4 - 0.25], axis=1)
    i, j, x, y = _lattice(10.25, 8.25, 8, 8, 0.125)
    parts["square_lattice"] = np.stack([x, y, -106 / 64 + ((i + j) % 2) / 64], axis=1)
    i, j, _, _ = _lattice(0, 0, 96, 3, 1)
    parts["thin_strip"] = np.stack([15.75 + (i + 2 * j) / 64, 14.75 + (i - 2 * j) / 64, -106 / 64 + ((i + j) % 2) / 64], axis=1)
    i, j, x, y = _lattice(46.0, 38.0, 8, 8, 0.125)
    parts["far_small"] = np.stack([x, y, -106 / 64 + (i + 2 * j + (i * j) % 3) / 64], axis=1)
    k = np.arange(30)
    z, r, s = E_PATCH["collinear"]
    r0, r1, t0, t1 = gr.patch_bounds(z, r, s)
    cx, cy = np.round(0.5 * (r0 + r1) * np.cos(0.5 * (t0 + t1)) * 64) / 64, np.round(0.5 * (r0 + r1) * np.sin(0.5 * (t0 + t1)) * 64) / 64
    parts["collinear"] = np.stack([cx + k / 64, cy - k / 64, np.full(30, -106 / 64)], axis=1)
    z, r, s = E_PATCH["copies"]
    r0, r1, t0, t1 = gr.patch_bounds(z, r, s)
    parts["copies"] = np.tile([[0.5 * (r0 + r1) * np.cos(0.5 * (t0 + t1)), 0.5 * (r0 + r1) * np.sin(0.5 * (t0 + t1)), -1.65]], (10, 1))
    parts["plain"] = np.concatenate([flat(rng, gr.DEFAULT, 3, 2, s, 30, G0) for s in (9, 11, 19, 21)] + [flat(rng, gr.DEFAULT, 2, 0, 4, 30, G0)])
    return parts


def _e_case(with_degenerate):
    rng = np.random.default_rng(61)
    pts, parts = _finish(rng, _e_parts(rng))
    if not with_degenerate:                    # the same rows in the same order, without the two patches: their neighbours' places stay
        drop = np.concatenate([parts.pop(k) for k in E_DEGENERATE])
        new = np.cumsum(~np.isin(np.arange(len(pts)), drop)) - 1
        pts, parts = np.delete(pts, drop, axis=0), {k: new[v] for k, v in parts.items()}
    return dict(pts=pts, parts=parts, params=gr.DEFAULT, patches={k: gr.patch_index(*v) for k, v in E_PATCH.items()},
                leave_out=tuple(gr.patch_index(*E_PATCH[k]) for k in E_DEGENERATE) if with_degenerate else (),
                claim="patches on exact lattices" + (", a collinear run and 10 copies of a point beside them" if with_degenerate else ""))


GROUPS = dict(
    E=dict(exact_lattices=functools.partial(_e_case, True), exact_lattices_alone=functools.partial(_e_case, False)),
    P=_p_cases(),
    S=dict(strides_mixed=_s_mixed),
    N=dict({f"n[{n}]": functools.partial(_n_size, n) for n in N_SIZES},
           **{k: functools.partial(_n_tile, k) for k in ("tile_64_patches", "tile_one_patch", "tile_two_alternating", "tile_unbinned", "one_patch_every_wave")}),
    L=dict(ties_mixed_lows=_l_ties, lows_late_places=_l_late, exactly_20=_l_exact, final_plane=_l_final_plane),
    R=dict(list_95=_r_list95, candidates_32=_r_cand32, dense_1500=functools.partial(_r_dense, 1500), dense_1501=functools.partial(_r_dense, 1501)))
NAMES = {name: group for group, cases in GROUPS.items() for name in cases}
LARGE = tuple(f"n[{n}]" for n in N_LARGE)


@functools.lru_cache(maxsize=None)
def get(name):
    """the case and the restatement's result at its parameters (computed once, left unchanged)"""
    case = GROUPS[NAMES[name]][name]()
    case["pts"] = np.ascontiguousarray(case["pts"], dtype=F)
    case["pts"].setflags(write=False)
    case["res"] = gr.segment(case["pts"], case["params"])
    return case

"""Seeded synthetic scenes for the ground segmentation (tests/test_ground.py, tests/test_gpu_ground.py): points placed patch by
patch of the concentric zone model, every coordinate with a small jitter (no exact lattices, except in `tied`), so that every
decision of the method stays clear of its threshold (ground_restatement.determined; asserted on the CPU for every scene).
A scene is float32 [n, 3] in a shuffled row order; `parts` names row sets the sanity tests look at."""
import numpy as np

import ground_restatement as gr


def in_patch(rng, zone, ring, sector, m, r_span=(0.06, 0.94), t_span=(0.06, 0.94)):
    """m points (x, y) inside a patch, away from its borders"""
    r0, r1, t0, t1 = gr.patch_bounds(zone, ring, sector)
    r = r0 + (r1 - r0) * rng.uniform(r_span[0], r_span[1], m)
    t = t0 + (t1 - t0) * rng.uniform(t_span[0], t_span[1], m)
    return r * np.cos(t), r * np.sin(t)


def flat(rng, zone, ring, sector, m, z=-1.7, sigma=0.01, **kw):
    x, y = in_patch(rng, zone, ring, sector, m, **kw)
    return np.stack([x, y, z + sigma * rng.standard_normal(m)], axis=1)


def ramp(rng, zone, ring, sector, m, slope, z_mid, sigma=0.01, **kw):
    """a plane rising outwards: z = z_mid + slope * (r - r_mid)"""
    x, y = in_patch(rng, zone, ring, sector, m, **kw)
    r0, r1, _, _ = gr.patch_bounds(zone, ring, sector)
    return np.stack([x, y, z_mid + slope * (np.hypot(x, y) - 0.5 * (r0 + r1)) + sigma * rng.standard_normal(m)], axis=1)


def radial_wall(rng, zone, ring, sector, m, z_lo, z_hi, sigma=0.003):
    """a thin vertical sheet along the patch's middle ray"""
    r0, r1, t0, t1 = gr.patch_bounds(zone, ring, sector)
    r = r0 + (r1 - r0) * rng.uniform(0.15, 0.85, m)
    t = 0.5 * (t0 + t1)
    off = sigma * rng.standard_normal(m)
    return np.stack([r * np.cos(t) - off * np.sin(t), r * np.sin(t) + off * np.cos(t), rng.uniform(z_lo, z_hi, m)], axis=1)


def box(rng, zone, ring, sector, m, z_lo=-1.7, z_hi=0.3):
    x, y = in_patch(rng, zone, ring, sector, m, r_span=(0.4, 0.6), t_span=(0.4, 0.6))
    return np.stack([x, y, rng.uniform(z_lo, z_hi, m)], axis=1)


def _finish(rng, parts):
    pts = np.concatenate(list(parts.values())).astype(np.float32)
    names = np.concatenate([np.full(len(v), k) for k, v in enumerate(parts.values())])
    perm = rng.permutation(len(pts))
    pts, names = pts[perm], names[perm]
    return pts, {k: np.flatnonzero(names == j) for j, k in enumerate(parts)}


def flat_boxes(seed=1):
    """flat ground at z = -1.7 in every near patch and some far ones, boxes standing on it"""
    rng = np.random.default_rng(seed)
    ground = [flat(rng, 0, r, s, 30) for r in range(2) for s in range(16)]
    ground += [flat(rng, 1, r, s, 24) for r in range(2) for s in range(32)]
    ground += [flat(rng, 2, 1, s, 20) for s in range(0, 54, 6)] + [flat(rng, 3, 0, s, 15) for s in range(0, 32, 8)]
    boxes = [box(rng, 0, 1, 3, 60), box(rng, 1, 0, 7, 50), box(rng, 1, 1, 20, 50), box(rng, 2, 1, 6, 40)]
    return _finish(rng, dict(ground=np.concatenate(ground), boxes=np.concatenate(boxes)))


def walls(seed=2):
    """a wall reaching below the ground in zone 0 (R-VPF removes it) and the same wall in zone 1 (R-VPF stops); a zone-0 patch
    that is nothing but a wall (R-VPF empties it); a zone-0 patch with points below -1.2 * sensor_height, one with all of its
    points below; a zone-1 patch whose only seed is one low outlier (NaN plane); slopes on both sides of 0.707"""
    rng = np.random.default_rng(seed)
    parts = dict(
        ground0=flat(rng, 0, 0, 2, 200), wall0=radial_wall(rng, 0, 0, 2, 400, -2.05, -1.2),
        ground1=flat(rng, 1, 1, 9, 200), wall1=radial_wall(rng, 1, 1, 9, 400, -2.05, -1.2),
        only_wall=radial_wall(rng, 0, 1, 5, 300, -2.0, -1.0),
        some_below=np.concatenate([flat(rng, 0, 1, 9, 150), flat(rng, 0, 1, 9, 6, z=-2.6, sigma=0.1)]),
        all_below=flat(rng, 0, 0, 11, 120, z=-2.5),
        outlier=np.concatenate([flat(rng, 1, 2, 4, 80), flat(rng, 1, 2, 4, 1, z=-8.0)]),
        gentle_far=ramp(rng, 2, 1, 10, 200, np.tan(np.radians(35.0)), -1.0, sigma=0.002),
        steep_far=ramp(rng, 2, 1, 30, 200, np.tan(np.radians(55.0)), -1.0, sigma=0.002),
        gentle_near=ramp(rng, 0, 1, 13, 200, -np.tan(np.radians(35.0)), -1.5, sigma=0.002),
        steep_near=ramp(rng, 0, 0, 7, 200, -np.tan(np.radians(55.0)), -1.0, sigma=0.002),
        plain=np.concatenate([flat(rng, 0, r, s, 25) for r in range(2) for s in (0, 15)] + [flat(rng, 3, 3, s, 25) for s in (0, 31)]))
    return _finish(rng, parts)


def platform(seed=3):
    """revert candidates: ramps that rise outwards through z >= 0 (upright, heading < 0, elevated) in the rings of interest.
    Ring 0 has ground only, three times as rough (sigma 0.03) as ring 1's ground (0.01): its flatness list carries over into
    ring 1 and lifts mu from about 1.3e-4 to about 1.2e-3, so that `middle` (sigma 0.02, flatness about 4e-4) is reverted with
    the carried list and would be rejected by ring 1's values alone.  Ring 1 has ground, a smooth candidate, the middle one,
    a rough one, a candidate of more than 1500 ground points and an elongated one; ring 2 has nothing; ring 3 has one ground
    patch and one candidate (one listed value: mu = 0, a division by zero)."""
    rng = np.random.default_rng(seed)
    parts = dict(
        ring0=np.concatenate([flat(rng, 0, 0, s, 60, sigma=0.03) for s in range(0, 16, 2)]),
        ring1=np.concatenate([flat(rng, 0, 1, s, 30) for s in (0, 1, 2, 3)]),
        smooth=ramp(rng, 0, 1, 6, 200, 0.2, 0.15, sigma=0.005),
        middle=ramp(rng, 0, 1, 14, 200, 0.2, 0.15, sigma=0.02),
        rough=ramp(rng, 0, 1, 8, 200, 0.2, 0.15, sigma=0.04),
        dense=ramp(rng, 0, 1, 10, 1700, 0.2, 0.15, sigma=0.04),
        long=ramp(rng, 0, 1, 12, 200, 0.2, 0.15, sigma=0.01, t_span=(0.4, 0.6)),
        ring3=flat(rng, 1, 1, 5, 40),
        lone=ramp(rng, 1, 1, 17, 150, 0.2, 0.3, sigma=0.01))
    return _finish(rng, parts)


def tied(seed=4):
    """many exactly equal z: ground at one float32 height, boxes on a few levels (the one scene on a lattice in z)"""
    rng = np.random.default_rng(seed)
    ground = np.concatenate([flat(rng, 0, r, s, 40, sigma=0.0) for r in range(2) for s in range(0, 16, 3)] +
                            [flat(rng, 1, 1, s, 40, sigma=0.0) for s in range(0, 32, 5)] + [flat(rng, 2, 0, s, 30, sigma=0.0) for s in (1, 20)])
    b = np.concatenate([box(rng, 0, 1, 3, 60), box(rng, 1, 1, 10, 60)])
    b[:, 2] = -1.7 + 0.3 * rng.integers(1, 7, len(b))
    return _finish(rng, dict(ground=ground, boxes=b))


def big_patch(seed=5, m=20000):
    """one patch of 20 000 points (ground and a box) next to ordinary ones"""
    rng = np.random.default_rng(seed)
    parts = dict(big=np.concatenate([flat(rng, 0, 1, 3, m - 500), box(rng, 0, 1, 3, 500)]),
                 rest=np.concatenate([flat(rng, 0, r, s, 30) for r in range(2) for s in (0, 8)]))
    return _finish(rng, parts)


def frame(seed=6, n=120000):
    """a full frame: ground with a gentle swell out to 70 m (some rows out of range), boxes and poles on it"""
    rng = np.random.default_rng(seed)
    m = n - 12000
    r, t = 70.0 * np.sqrt(rng.uniform(0.0, 1.0, m)), rng.uniform(0.0, 2 * np.pi, m)
    x, y = r * np.cos(t), r * np.sin(t)
    ground = np.stack([x, y, -1.7 + 0.05 * np.sin(0.1 * x) * np.cos(0.13 * y) + 0.01 * rng.standard_normal(m)], axis=1)
    cx, cy = rng.uniform(-50, 50, 60), rng.uniform(-50, 50, 60)
    k = rng.integers(0, 60, 12000)
    objects = np.stack([cx[k] + rng.uniform(-1, 1, 12000), cy[k] + rng.uniform(-1, 1, 12000), rng.uniform(-1.7, 0.8, 12000)], axis=1)
    return _finish(rng, dict(ground=ground, objects=objects))


def edges(seed=7):
    """the edges of the binning: rows exactly on r = 1 (out), r = 64 (in) and on every zone boundary, y = +-0 with x > 0 (the
    last sector) and with x < 0, rows out of range and rows with NaN / inf; a patch of 9 points and one of 10.  Not shuffled."""
    rng = np.random.default_rng(seed)
    z = np.float32(-1.7)
    rows = [[1.0, 0.0, z], [0.0, 1.0, z], [64.0, 0.0, z], [0.0, -64.0, z], [63.0, 1e-3, z], [0.5, 0.5, z], [100.0, 3.0, z], [0.0, 0.0, z]]
    for b in gr.LO[1:]:
        rows += [[b, 0.0, z], [0.0, b, z], [-b, 0.0, z], [0.0, -b, z], [np.nextafter(np.float32(b), np.float32(0)), 0.0, z]]
    rows += [[5.0, 0.0, z], [5.0, -0.0, z], [-5.0, 0.0, z], [-5.0, -0.0, z], [20.0, 0.0, z], [20.0, -0.0, z], [-20.0, -0.0, z], [40.0, -0.0, z]]
    rows += [[np.nan, 1.0, z], [3.0, np.inf, z], [3.0, 3.0, np.nan], [-np.inf, np.nan, z], [3.0, 3.0, -np.inf]]
    parts = dict(special=np.asarray(rows, dtype=np.float64), nine=flat(rng, 3, 1, 4, 9), ten=flat(rng, 3, 1, 9, 10),
                 last_sector=flat(rng, 0, 0, 15, 30, t_span=(0.5, 0.999)), ground=flat(rng, 1, 0, 0, 30, t_span=(0.001, 0.5)))
    pts = np.concatenate(list(parts.values())).astype(np.float32)
    at, where = 0, {}
    for k, v in parts.items():
        where[k] = np.arange(at, at + len(v))
        at += len(v)
    return pts, where


SMALL = dict(flat_boxes=flat_boxes, walls=walls, platform=platform, tied=tied)
LARGE = dict(big_patch=big_patch, frame=frame)
ALL = dict(SMALL, **LARGE, edges=edges)

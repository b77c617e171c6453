"""The inputs the box tests share (tests/test_boxes.py on the CPU, tests/test_gpu_boxes.py on the GPU): rectangle outlines with
a known yaw, the tie cases, and the labelled clouds of the shapes list.  Each tie case's claim is checked in
tests/test_boxes.py against the restatement's per-direction scores.  Not a test module."""
import numpy as np

F = np.float32
STEP_DEG = 1.0            # of box_directions(90)


def outline(length, width, yaw_deg, centre, n, sides=4, z=(0.0, 1.5)):
    """n points evenly spaced along the outline of a length x width rectangle (corners included), turned by yaw_deg about its
    centre: all four sides, or the two that meet at the corner (+length / 2, +width / 2) -- an L.  float64 in, float32 out."""
    hl, hw = length / 2.0, width / 2.0
    if sides == 4:
        corners = np.array([[hl, hw], [-hl, hw], [-hl, -hw], [hl, -hw], [hl, hw]])
    else:
        corners = np.array([[-hl, hw], [hl, hw], [hl, -hw]])
    seg = np.linalg.norm(np.diff(corners, axis=0), axis=1)
    at = np.linspace(0.0, seg.sum(), n)
    edge = np.minimum(np.searchsorted(np.cumsum(seg), at, side="left"), len(seg) - 1)
    t = (at - (np.cumsum(seg) - seg)[edge]) / seg[edge]
    local = corners[edge] + t[:, None] * (corners[edge + 1] - corners[edge])
    local[[0, -1]] = corners[0], corners[-1]
    for k in range(1, len(corners) - 1):             # every corner is a point of the outline
        local[np.argmin(np.abs(at - np.cumsum(seg)[k - 1]))] = corners[k]
    a = np.deg2rad(yaw_deg)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    xy = local @ rot.T + np.asarray(centre, np.float64)[None, 0:2]
    zz = np.linspace(z[0], z[1], n)
    return np.concatenate([xy, zz[:, None]], axis=1).astype(F)


def truth_cases(count, seed, sides, on_grid=False):
    """`count` seeded outlines: length 1.5 - 5 m, width 1 - 2.2 m, 30 - 1500 points, any yaw (on_grid: a whole number of
    degrees), centres up to 60 m out.  -> list of dict(points, length, width, yaw)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        length, width = rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2)
        yaw = float(rng.integers(0, 360)) if on_grid else rng.uniform(0.0, 360.0)
        r, phi = rng.uniform(0.0, 60.0), rng.uniform(0.0, 2 * np.pi)
        n = int(rng.integers(30, 1501))
        out.append(dict(points=outline(length, width, yaw, (r * np.cos(phi), r * np.sin(phi)), n, sides), length=length, width=width, yaw=yaw))
    return out


def cyclic_steps(k, yaw_deg, A=90):
    """how many steps direction k lies from yaw_deg mod 90 degrees, cyclically"""
    step = 90.0 / A
    d = abs(k * step - yaw_deg % 90.0)
    return min(d, 90.0 - d) / step


def tie_near():
    """Two rows along direction 30 of 90: both lie on a corner of every bounding rectangle, so `near` is 2 in every direction
    and the area decides -- it is smallest where the rectangle collapses onto the line, at k = 30."""
    a = np.deg2rad(30.0)
    p = np.array([[-2 * np.cos(a), -2 * np.sin(a), 0.0], [2 * np.cos(a), 2 * np.sin(a), 1.0]])
    return dict(points=p.astype(F), A=90, delta=0.1, k=30)


SYM_C, SYM_S = 19.0 / 32.0, 103.0 / 128.0           # c * c + s * s = 1.00006..., both with few bits: every product below is exact


def symmetric_directions():
    """three directions with c[A - k] = s[k] bit for bit (k = 1, 2), few mantissa bits each"""
    return np.array([[1.0, 0.0], [SYM_C, SYM_S], [SYM_S, SYM_C]], F)


def tie_area():
    """A point set symmetric under x <-> y -- a stick along direction 1 and its mirror image, along direction 2, centroid
    (0, 0) -- under the symmetric direction table and a delta that makes every row near in every direction: `near` ties
    everywhere, the areas of directions 1 and 2 are equal bit for bit (every product and sum is exact in float32) and smaller
    than direction 0's, so the lower k, 1, wins."""
    t = np.arange(-4, 5, dtype=np.float64)
    stick = np.stack([t * SYM_C, t * SYM_S, 0.25 * t], axis=1)
    mirror = stick[:, [1, 0, 2]]
    return dict(points=np.concatenate([stick, mirror]).astype(F), dirs=symmetric_directions(), delta=1e3, k=1)


SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)


def blobs(sizes, seed, span=40.0, ground=500, noise=100, centre=(0.0, 0.0)):
    """One labelled cloud: segment j (label j) has sizes[j] rows scattered over a random rectangle's outline and inside, plus
    ground (-1e8) and noise (-1) rows, everything shuffled together.  -> (points float32 [n, 3], labels float32 [n])"""
    rng = np.random.default_rng(seed)
    pts, lab = [], []
    for j, size in enumerate(sizes):
        c = rng.uniform(-span, span, 2) + np.asarray(centre)
        yaw, ext = rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 4.0, 2)
        local = rng.uniform(-1.0, 1.0, (size, 2)) * ext
        edge = rng.random(size) < 0.7                 # most rows on the outline, like a LiDAR cluster
        side = rng.integers(0, 2, size)
        local[edge, side[edge]] = np.sign(local[edge, side[edge]]) * ext[side[edge]]
        rot = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        pts.append(np.concatenate([local @ rot.T + c, rng.uniform(-1.0, 1.0, (size, 1))], axis=1))
        lab.append(np.full(size, float(j)))
    pts.append(np.concatenate([rng.uniform(-span, span, (ground, 2)), np.full((ground, 1), -1.7)], axis=1))
    lab.append(np.full(ground, -1e8))
    pts.append(rng.uniform(-span, span, (noise, 3)))
    lab.append(np.full(noise, -1.0))
    pts, lab = np.concatenate(pts).astype(F), np.concatenate(lab).astype(F)
    mix = rng.permutation(len(pts))
    return pts[mix], lab[mix]

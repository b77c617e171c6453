"""The inputs of tests/test_gpu_ego_map.py (NumPy only), so that tests/test_ego_map_cases.py can check on the CPU that every
case is the case its name claims.  The ego-motion estimator's voxel map (csrc/ego.hip) taken on its own: probe chains, a
wrap, full tables, the order and the caps inside a voxel, tile and chunk seams, coordinates on voxel faces, the crop's and
the prune's edges, and the decisions of the registration (ties, the gate, the 27 voxels, fewer than 3 correspondences).

The one piece of the implementation that building inputs needs is restated here: `home`, the slot a key's probe starts at.
It CHOOSES voxels; no result is judged with it -- the yardstick (ego_motion_restatement.py) knows no hash and no slot.

    MAP_CASES[name]()   -> dict(constants, frames=[(points float32 [n,3], pose float64 [4,4]), ...], ...)   map_add per frame
    DS_CASES[name]()    -> dict(constants, points)                                                          downsample
    REG_CASES[name]()   -> dict(constants, frames (the map), source, guess, sigma)                           register_step
"""
import functools

import numpy as np

import ego_motion_restatement as rest

F = np.float32
BASE = dict(map_capacity=1024, max_range=100.0, min_range=1.0)      # v = 1 m: x / v is exact
MASK = 1023
REACH = 57                  # voxels -57 .. 57 per axis: every centre within 99.6 m of the origin
EYE = np.eye(4)


def home(key, mask):
    """csrc/ego.hip hash_key: where the probe of `key` starts in a table of mask + 1 slots"""
    k = np.asarray(key).astype(np.uint64)
    return ((k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)) & np.uint64(mask)


def keys_of(points, size):
    return rest.pack(rest.voxel_coords(points, size))


def longest_displacement(keys, mask):
    """slots walked past the home slot by the unluckiest key when `keys` enter an empty table one after the other"""
    taken = np.zeros(mask + 1, bool)
    worst = 0
    for h in home(keys, mask).tolist():
        d = 0
        while taken[(h + d) & mask]:
            d += 1
        taken[(h + d) & mask] = True
        worst = max(worst, d)
    return worst


@functools.lru_cache(maxsize=None)
def grid(reach=REACH, mask=MASK):
    """every voxel of [-reach, reach]^3 in a seeded order, and its home slot"""
    a = np.arange(-reach, reach + 1)
    ijk = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[np.random.default_rng(7).permutation(len(ijk))]
    return ijk, home(rest.pack(ijk), mask).astype(np.int64)


def voxels_at_home(slot, count, keep=None, reach=REACH, mask=MASK):
    """`count` voxels (int64 [count,3]) whose probe starts at `slot`; keep: a filter on the voxels' centres"""
    ijk, h = grid(reach, mask)
    sel = ijk[h == slot]
    if keep is not None:
        sel = sel[keep(sel + 0.5)]
    assert len(sel) >= count, (slot, len(sel), count)
    return sel[:count]


def centre(ijk, size=1.0, at=0.5):
    """a point of every voxel: (ijk + at) * size, exact in float32 for the sizes used here"""
    out = (np.asarray(ijk, np.float64) + at) * size
    assert np.array_equal(out.astype(F).astype(np.float64), out)
    return out.astype(F)


def translation(x, y, z):
    T = np.eye(4)
    T[0:3, 3] = (x, y, z)
    return T


def rotation_z(deg, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T[0:2, 0:2] = [[c, -s], [s, c]]
    T[0:3, 3] = t
    return T


def step(x, towards):
    """one float32 step from x towards `towards`"""
    return np.nextafter(F(x), F(towards))


def restated_maps(case):
    """the restatement's map after every frame of a map case -> [snapshot, ...]"""
    c = dict(rest.DEFAULTS, **{k: v for k, v in case["constants"].items() if k in rest.DEFAULTS})
    voxel = c["voxel_size"] if c["voxel_size"] > 0 else c["max_range"] / 100.0
    m = rest.VoxelMap(voxel, c["max_points_per_voxel"], c["max_range"])
    out = []
    for pts, pose in case["frames"]:
        m.update(pts, pose)
        out.append(m.snapshot())
    case["_map"] = m
    return out


# ============================================================================================ A. the table
def chain(slot, count=40):
    """`count` voxels of one home slot, one point each; a second frame adds a point to every one of them (in another order);
    the registration of the first points must find every one of them at the end of its chain"""
    ijk = voxels_at_home(slot, count)
    second = centre(ijk, at=0.25)[np.random.default_rng(slot).permutation(count)]
    return dict(constants=dict(BASE, max_points=64), voxels=ijk, home=slot, frames=[(centre(ijk), EYE), (second, EYE)],
                source=centre(ijk), guess=EYE, sigma=1.0)


def chain_pruned_middle():
    """30 voxels of one home slot, entered alternately near (within max_range of (60, 0, 0)) and far from it (beyond); the
    second frame's pose stands at (60, 0, 0), so every second voxel of the chain leaves.  (The slots themselves are handed
    out by arrival; what is certain is that 15 of the 30 keys that shared one chain are gone and 15 must still be found.)"""
    t = np.array([60.0, 0.0, 0.0])
    near = voxels_at_home(300, 15, lambda c: np.linalg.norm(c - t, axis=1) < 95.0)
    far = voxels_at_home(300, 15, lambda c: np.linalg.norm(c - t, axis=1) > 105.0)
    ijk = np.stack([near, far], 1).reshape(30, 3)
    fresh = np.array([[1.5, 2.5, 0.5], [2.5, 2.5, 0.5], [3.5, -2.5, 1.5], [-4.5, 2.5, 0.5], [5.5, 7.5, -0.5]], F)   # sensor coordinates
    frames = [(centre(ijk), EYE), (fresh, translation(*t))]
    world = (fresh.astype(np.float64) + t).astype(F)
    return dict(constants=dict(BASE, max_points=64), voxels=ijk, near=near, far=far, home=300, frames=frames,
                source=np.concatenate([centre(near), world]), guess=EYE, sigma=1.0)


def load(count, seed):
    """`count` seeded-random voxels in one frame, a second point for every one in the next; the registration of the first
    points against it must find every one of them"""
    ijk, _ = grid()
    pick = ijk[np.random.default_rng(seed).choice(len(ijk), count, replace=False)]
    second = centre(pick, at=0.75)[np.random.default_rng(seed + 1).permutation(count)]
    return dict(constants=dict(BASE, max_points=1024), voxels=pick, frames=[(centre(pick), EYE), (second, EYE)],
                source=centre(pick), guess=EYE, sigma=1.0)


def full_plus_one():
    """1025 points at least 1 m apart inside the crop: 1025 voxels of frame_ds, 1025 voxels of the map -- one too many"""
    ijk, _ = grid()
    ijk = ijk[np.linalg.norm(ijk + 0.5, axis=1) > 2.0]
    pick = ijk[np.random.default_rng(11).choice(len(ijk), 1025, replace=False)]
    return dict(constants=dict(BASE, max_points=2048), points=centre(pick))


def coord_range():
    """voxel_size 1e-4: floor(x / 0.5e-4) of x = 60 m is 1.2e6, beyond the 2^20 - 2 a key holds; the rest of the frame stays
    within 50 m (< 52.4 m = (2^20 - 2) * 0.5e-4) and passes without that point.  Rows of NaN and +-inf ride along."""
    rng = np.random.default_rng(12)
    pts = rng.uniform(-25.0, 25.0, (300, 3)).astype(F)
    pts = pts[np.linalg.norm(pts, axis=1) > 2.0]
    bad = np.array([[np.nan, 1, 1], [3, np.inf, 1], [-np.inf, 2, 2], [2, 2, np.nan], [np.inf, np.inf, np.inf]], F)
    return dict(constants=dict(BASE, voxel_size=1e-4, max_points=512), good=pts, beyond=np.array([[60.0, 1.0, 1.0]], F), bad=bad)


# ============================================================================================ B. order, caps, seams
SEAM_ROWS = np.array(sorted([0, 1] + [256 * k + d for k in range(1, 9) for d in (-1, 0, 1)])[:25])
CAP_VOXEL = np.array([3, 4, 5])


def cap_one_frame(per_voxel):
    """one frame of 2100 rows; 25 of them, on both sides of every 256-row tile of map_append_kernel, fall into one voxel,
    each at a place of its own; the other rows into 300 other voxels (several rows each: their caps count too)"""
    rng = np.random.default_rng(20)
    n = 2100
    ijk, _ = grid()
    others = ijk[~(ijk == CAP_VOXEL).all(1)][:300]
    pts = (others[rng.integers(0, len(others), n)] + rng.integers(1, 64, (n, 3)) / 64.0).astype(F)
    pts[SEAM_ROWS] = (CAP_VOXEL + (np.arange(25)[:, None] + 1.0) / 32.0 * np.array([1.0, 0.5, 0.25])).astype(F)
    return dict(constants=dict(BASE, max_points=4096, max_points_per_voxel=per_voxel), frames=[(pts, EYE)],
                voxel=CAP_VOXEL, rows=SEAM_ROWS)


def cap_two_frames():
    """per_voxel 20: voxel A holds 18 and the next frame brings 5 (the two lowest-indexed enter), B holds 20 and gets 3
    (nothing changes), C is new and gets exactly 20; the rows of the second frame are shuffled among 400 others"""
    rng = np.random.default_rng(21)
    A, B, C = np.array([10, 0, 0]), np.array([-10, 5, 0]), np.array([0, -20, 3])
    inside = lambda v, k: (v + rng.integers(1, 256, (k, 3)) / 256.0).astype(F)     # noqa: E731
    ijk, _ = grid()
    others = ijk[~((ijk == A).all(1) | (ijk == B).all(1) | (ijk == C).all(1))][:200]
    first = np.concatenate([inside(A, 18), inside(B, 22), inside(others[rng.integers(0, 200, 100)], 100)])
    first = first[rng.permutation(len(first))]
    second = np.concatenate([inside(A, 5), inside(B, 3), inside(C, 20), inside(others[rng.integers(0, 200, 400)], 400)])
    second = second[rng.permutation(len(second))]
    return dict(constants=dict(BASE, max_points=1024), frames=[(first, EYE), (second, EYE)], A=A, B=B, C=C)


FACE_K = (-3, -1, 0, 1, 57)


def faces(voxel):
    """a coordinate exactly on a voxel face (float32(k v) for k in FACE_K, and -0.0) and one float32 step below it, on every
    axis in turn; the other two coordinates sit mid-voxel.  v = 1: the faces are exact; v = 0.3: they are not, and the voxel is
    whatever floor(float64(x) / 0.3) says"""
    rows = []
    for axis in range(3):
        for k in FACE_K:
            x = F(k * voxel)
            for val in (x, step(x, -np.inf), step(x, np.inf)):
                p = np.array([10.5, 20.5, 30.5], F) * F(voxel)
                p = np.roll(p, axis)
                p[axis] = val
                rows.append(p)
        p = np.roll(np.array([10.5, 20.5, 30.5], F) * F(voxel), axis)
        p[axis] = F(-0.0)
        rows.append(p)
    return dict(constants=dict(BASE, voxel_size=voxel, max_points=64), frames=[(np.stack(rows), EYE)])


FLIP_POSE = rotation_z(37.0, (0.25, -1.5, 0.125))


def rounding_flips():
    """points whose image under FLIP_POSE lies a hair below a voxel face in fp64 and ON it once rounded to float32: the voxel
    is the float32 image's.  Searched, not drawn: for every face k the float32 neighbours of the x (or y) that solves
    R p + t = k are tried and those that flip are kept."""
    T = FLIP_POSE
    rows = []
    for axis in (0, 1):
        for k in range(-40, 41):
            if k == 0:
                continue
            other = F(3.25 + 0.5 * (k % 7))
            # T[axis,0] * a + T[axis,1] * other + t = k
            a0 = F((k - T[axis, 3] - T[axis, 1] * float(other)) / T[axis, 0])
            a = a0
            for _ in range(6):
                a = step(a, -np.inf)
            for _ in range(13):
                p = np.array([a, other, F(0.5 + (k % 5))], F)
                x64 = rest.move(T, p[None])[0]
                if (np.floor(x64) != np.floor(x64.astype(F).astype(np.float64))).any():
                    rows.append(p)
                a = step(a, np.inf)
    pts = np.stack(rows)
    return dict(constants=dict(BASE, max_points=1024), frames=[(pts, T)], pose=T)


PRUNE_T = np.array([3.0, -4.0, 12.0])
_EDGE_E = [(-60, 80, 0), (0, 0, -100), (-80, 0, -60), (60, 80, 0), (0, -60, -80), (0, 80, -60), (-60, 0, -80), (0, -80, -60),
           (-48, -36, -80), (-36, 48, -80)]


def prune_edge():
    """frame 0 (identity) enters one point per voxel; frame 1 brings no point and a pose at PRUNE_T.  Voxels `on`: the first
    point exactly max_range from PRUNE_T (kept: the test is `>`); `beyond`: one float32 step farther (dropped); `first_out`:
    first point out of range, later ones in range (dropped whole); `first_in`: the reverse (kept whole)."""
    on, beyond = [], []
    for j, e in enumerate(_EDGE_E):
        p = (PRUNE_T + e).astype(F)
        if j % 2:
            a = int(np.argmax(np.abs(e)))
            p[a] = step(p[a], np.inf if e[a] > 0 else -np.inf)
            beyond.append(p)
        else:
            on.append(p)
    # a voxel the sphere passes through: e = (-70.x, 70.9, 0.5)
    inn, out = (PRUNE_T + (-70.5, 70.9, 0.5)).astype(F), (PRUNE_T + (-70.9, 70.9, 0.5)).astype(F)
    # ... and another: e = (-50.5, -62.5, -59.x)
    inn2, out2 = (PRUNE_T + (-50.5, -62.5, -59.5)).astype(F), (PRUNE_T + (-50.5, -62.5, -59.9)).astype(F)
    pts = np.stack(on + beyond + [out, inn, inn, inn2, out2, out2])
    return dict(constants=dict(BASE, max_points=64), frames=[(pts, EYE), (np.zeros((0, 3), F), translation(*PRUNE_T))],
                on=np.stack(on), beyond=np.stack(beyond), first_out=(out, inn), first_in=(inn2, out2))


def prune_d2(p, t=PRUNE_T):
    """the squared distance as the kernel forms it: fp64 from the float32 point"""
    e = np.asarray(p, F).astype(np.float64) - t
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


SIZES = (0, 1, 255, 256, 257, 1025)


def sizes():
    """map_add of 0 (prune only), 1, 255, 256, 257 and 1025 points, one after the other onto one map, 400 voxels in all"""
    rng = np.random.default_rng(22)
    ijk, _ = grid()
    frames = [((ijk[rng.integers(0, 400, n)] + rng.integers(1, 64, (n, 3)) / 64.0).astype(F).reshape(n, 3), EYE) for n in SIZES]
    return dict(constants=dict(BASE, max_points=2048), frames=frames)


def three_frames():
    """a small static scene seen from three places: 1500 points on the walls of a 30 x 20 x 4 m room"""
    rng = np.random.default_rng(23)
    frames = []
    for j in range(3):
        u = rng.uniform(-0.5, 0.5, (1500, 3)) * (30.0, 20.0, 4.0)
        face = rng.integers(0, 3, 1500)
        for k in range(3):
            u[face == k, k] = np.sign(u[face == k, k]) * 0.5 * (30.0, 20.0, 4.0)[k]
        frames.append((u - (0.3 * j, 0.1 * j, 0.0)).astype(F))
    return dict(constants=dict(BASE, map_capacity=1 << 14, max_points=2048), points=frames)


MAP_CASES = {
    "chain_40": lambda: chain(500),
    "chain_40_wrap": lambda: chain(MASK),
    "chain_pruned_middle": chain_pruned_middle,
    "load_half": lambda: load(512, 30),
    "load_full": lambda: load(1024, 31),
    "cap_one_frame[1]": lambda: cap_one_frame(1),
    "cap_one_frame[3]": lambda: cap_one_frame(3),
    "cap_one_frame[20]": lambda: cap_one_frame(20),
    "cap_two_frames": cap_two_frames,
    "faces[1.0]": lambda: faces(1.0),
    "faces[0.3]": lambda: faces(0.3),
    "rounding_flips": rounding_flips,
    "prune_edge": prune_edge,
    "sizes": sizes,
}


# ============================================================================================ C. the down-sampling
DS_SEAM_N = (1023, 1024, 1025, 2049, 5000)


def ds_seams(n):
    """n rows in about n / 2.5 voxels of 0.5 v, one to four rows each, in shuffled order, all within 8 m: a voxel's rows lie
    in different chunks of ds_compact_kernel's threads (chunk = ceil(n / 1024)), and many 1.5 v voxels hold several"""
    rng = np.random.default_rng(40 + n)
    a = np.arange(-16, 16)
    ijk = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[np.linalg.norm((ijk + 0.5) * 0.5, axis=1) > 1.5]
    ijk = ijk[rng.permutation(len(ijk))]
    owner = np.repeat(np.arange(n), rng.integers(1, 5, n))[:n][rng.permutation(n)]      # the voxel of every row
    pts = ((ijk[owner] + rng.integers(1, 32, (n, 3)) / 32.0) * 0.5).astype(F)
    return dict(constants=dict(BASE, max_points=5000), points=pts, owner=owner, chunk=(n + 1023) // 1024)


def straddling_voxels(owner, chunk):
    """the voxels whose lowest row and a higher row of theirs belong to different threads of the compaction"""
    out = []
    for o in np.unique(owner):
        rows = np.nonzero(owner == o)[0]
        if len(rows) > 1 and rows[0] // chunk != rows[-1] // chunk:
            out.append(int(o))
    return out


MAX_ON = [(60, 80, 0), (36, 48, 80), (100, 0, 0), (0, -100, 0), (-28, 96, 0), (64, 48, -60)]
MIN_ON = [(1, 0, 0), (0, -1, 0), (0, 0, 1)]


def ds_crop_edge():
    """rows exactly min_range / max_range from the sensor (r^2 == 1, == 10000 in fp64: excluded by the strict crop), one
    float32 step inside the crop next to each (included) and one step outside (excluded); rows of NaN and +-inf; filler"""
    rows, kind = [], []
    for e in MAX_ON + MIN_ON:
        p = np.array(e, F)
        a = int(np.argmax(np.abs(p)))
        big = abs(p[a]) > 1.5
        inward = p.copy()
        inward[a] = step(p[a], 0.0 if big else np.sign(p[a]) * 2.0)
        outward = p.copy()
        outward[a] = step(p[a], np.sign(p[a]) * 1000.0 if big else 0.0)
        rows += [p, inward, outward]
        kind += ["on", "inside", "outside"]
    for bad in ([np.nan, 1, 1], [3, np.inf, 1], [-np.inf, 2, 2], [2, 2, np.nan], [np.inf, -np.inf, np.inf]):
        rows.append(np.array(bad, F))
        kind.append("bad")
    rng = np.random.default_rng(41)
    fill = rng.uniform(-30, 30, (200, 3)).astype(F)
    order = rng.permutation(len(rows) + len(fill))
    pts = np.concatenate([np.stack(rows), fill])[order]
    kind = np.array(kind + ["fill"] * len(fill))[order]
    return dict(constants=dict(BASE, max_points=512), points=pts, kind=kind)


def ds_collisions(size_factor):
    """512 rows in 512 different voxels of size_factor * v, 300 of which start their probe at one slot of the 1024-slot
    scratch table (max_points = 512: tcap = 1024, load exactly one half).  0.5: the first pass; 1.5: the second pass, every row
    alone in its 1.5 v voxel, so that all 512 reach it"""
    reach = 50 if size_factor == 0.5 else 40
    keep = lambda c: (np.linalg.norm(c * size_factor, axis=1) > 2.0) & (np.linalg.norm(c * size_factor, axis=1) < 99.0)   # noqa: E731
    same = voxels_at_home(77, 300, keep, reach=reach)
    ijk, h = grid(reach)
    rest_ = ijk[(h != 77) & keep(ijk + 0.5)][:212]
    rng = np.random.default_rng(42)
    pts = centre(np.concatenate([same, rest_]), size_factor)[rng.permutation(512)]
    return dict(constants=dict(BASE, max_points=512), points=pts, size=size_factor, home=77)


def ds_all_one_voxel():
    rng = np.random.default_rng(43)
    return dict(constants=dict(BASE, max_points=3000), points=(10.0 + rng.integers(1, 128, (3000, 3)) / 256.0).astype(F))


def ds_all_distinct():
    ijk, _ = grid(40)
    r = np.linalg.norm((ijk + 0.5) * 1.5, axis=1)
    ijk = ijk[(r > 2.0) & (r < 99.0)][:3000]
    assert len(ijk) == 3000
    return dict(constants=dict(BASE, max_points=3000), points=centre(ijk, 1.5))


DS_CASES = dict({f"ds_seams[{n}]": functools.partial(ds_seams, n) for n in DS_SEAM_N},
                ds_crop_edge=ds_crop_edge, **{"ds_collisions[0.5v]": lambda: ds_collisions(0.5), "ds_collisions[1.5v]": lambda: ds_collisions(1.5)},
                ds_all_one_voxel=ds_all_one_voxel, ds_all_distinct=ds_all_distinct)


# ============================================================================================ D. the registration's decisions
def anchors(count, seed, spread=30, avoid=()):
    """`count` map points on the 0.25 m lattice, each in a voxel of its own at least 4 voxels (chessboard distance) from the
    next, from the cases' special points around the origin (one |coordinate| >= 8) and from `avoid`: a source put ON one has
    residual 0 and no other candidate"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        c = rng.integers(-spread, spread, 3)
        if np.abs(c).max() < 8 or any(np.abs(c - np.floor(o)).max() < 4 for o in list(out) + list(avoid)):
            continue
        out.append(c)
    return (np.array(out) + rng.integers(1, 4, (count, 3)) / 4.0).astype(F)


def reg(frames, source, sigma, guess=EYE, max_iterations=1, **more):
    return dict(constants=dict(BASE, max_points=2048, max_iterations=max_iterations, **more.pop("constants", {})), frames=frames,
                source=np.asarray(source, F).reshape(-1, 3), guess=np.array(guess, np.float64), sigma=float(sigma), **more)


def tie_voxels():
    """four sources exactly midway between two map points of different neighbouring voxels (x, y, z, and the diagonal): lattice
    coordinates, identity guess, every difference and square exact.  The point of the EARLIER voxel offset wins"""
    A = anchors(20, 50)
    c = np.array([[0.0, 1.5, 1.5], [-1.5, -3.0, 1.5], [1.5, -2.5, -2.0], [-3.0, 3.0, -3.0]])     # the sources: on a face
    d = np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0.5]])
    first, second = c - d, c + d                       # offset -1 is searched before offset 0
    mp = np.concatenate([A, second, first]).astype(F)   # (entered in the other order: insertion does not decide here)
    return reg([(mp, EYE)], np.concatenate([A, c]), 1.0, ties=c.astype(F), winners=first.astype(F), losers=second.astype(F))


def tie_insertion():
    """two map points of ONE voxel equidistant from a source: the earlier insertion wins -- the lower row of one frame, and
    the point of the earlier frame over the lower row of a later one"""
    A = anchors(20, 51)
    c = np.array([[0.5, 1.5, 1.5], [-1.5, -2.5, 1.5], [1.5, -2.5, -1.5], [-2.5, 2.5, -2.5]])
    d = np.array([[0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [0.25, 0, 0]])
    first, second = c + d, c - d
    f0 = np.concatenate([A, first[:3], second[:3], first[3:]]).astype(F)
    f1 = second[3:].astype(F)                            # row 0 of a LATER frame
    return reg([(f0, EYE), (f1, EYE)], np.concatenate([A, c]), 1.0, ties=c.astype(F), winners=first.astype(F), losers=second.astype(F))


def gate_edge():
    """sigma 0.5: (3 sigma)^2 = 2.25 exactly.  Six sources 1.5 m from their only map point (d^2 == 2.25: no correspondence); one
    whose map point is 2^-52 m closer (x = 2^-52 in the next voxel: d^2 is the fp64 below 2.25: a correspondence)"""
    on_src = np.array([[11.5, 0.5, 0.5], [-10.5, 3.5, 0.5], [4.5, 12.5, -3.5], [-5.5, -11.5, 2.5], [8.5, -8.5, 6.5], [-9.5, 9.5, -6.5]])
    A = anchors(6, 52, avoid=on_src)
    on_map = on_src - [1.5, 0, 0]
    below_src, below_map = np.array([[1.5, 0.5, 0.5]]), np.array([[2.0 ** -52, 0.5, 0.5]])
    mp = np.concatenate([A, on_map, below_map]).astype(F)
    return reg([(mp, EYE)], np.concatenate([A, on_src, below_src]), 0.5, on=(on_src.astype(F), on_map.astype(F)),
               below=(below_src.astype(F), below_map.astype(F)))


def only_27(adjacent):
    """four sources whose only map point is two voxels away, 1.75 m, well inside the gate of sigma = 1 (9 m^2): not found.
    adjacent: the same map points 0.5 m nearer, in the neighbouring voxel: found"""
    A = anchors(6, 53)
    src = np.array([[0.5, 0.5, 0.5], [-3.5, 2.5, 1.5], [2.5, -3.5, -1.5], [-1.5, -2.5, 3.5]])
    off = np.array([[1.75, 0, 0], [0, 1.75, 0], [0, 0, -1.75], [-1.75, 0, 0]])
    if adjacent:
        off = off / 1.75 * 1.25
    mp = np.concatenate([A, src + off]).astype(F)
    return reg([(mp, EYE)], np.concatenate([A, src]), 1.0, lonely=src.astype(F), expect=6 + (4 if adjacent else 0))


def twentieth_point():
    """a voxel filled to 20 points whose LAST point is the one nearest to a source (four such voxels)"""
    A = anchors(6, 54)
    rng = np.random.default_rng(54)
    vox = np.array([[0, 0, 0], [-3, 2, 1], [2, -3, -2], [-2, -3, 3]])
    cells, src = [], []
    for v in vox:
        far = v + np.array([0.0625, 0.0625, 0.0625]) + rng.integers(0, 8, (19, 3)) / 64.0     # the first 19: in the low corner
        last = v + np.array([0.75, 0.75, 0.75])
        cells.append(np.concatenate([far, last[None]]))
        src.append(last + [0.125, 0.0, 0.0])
    mp = np.concatenate([A] + cells).astype(F)
    return reg([(mp, EYE)], np.concatenate([A, np.array(src)]), 1.0, voxels=vox)


FEW_GUESS = rotation_z(3.0, (0.5, -0.25, 0.125))


def few(count):
    """`count` sources, each near a map point under a guess that is no identity.  2: the guess comes back bit for bit;
    3 (not collinear): a step"""
    mp = np.array([[5.5, 1.5, 0.5], [-4.5, 6.5, 1.5], [2.5, -7.5, -1.5], [10.5, 10.5, 3.5], [-12.5, -3.5, 2.5]], F)
    want = mp[:count].astype(np.float64) + np.array([[0.125, -0.0625, 0.03125]])
    src = rest.move(rest.rigid_inverse(FEW_GUESS), want)
    return reg([(mp, EYE)], src, 1.0, FEW_GUESS)


def own_points():
    """source = the map's own points, identity guess: every residual is 0, dx = 0, the pose is the guess bit for bit"""
    A = anchors(40, 55)
    return reg([(A, EYE)], A, 1.0)


M_SEAMS = (1, 511, 512, 513, 1025)


def m_seams(m):
    """m sources 5 cm from a map point each (1200 map voxels, map_capacity 4096): m across the 512 threads of the one
    workgroup; one iteration"""
    rng = np.random.default_rng(56)
    ijk, _ = grid(20)
    mp = (ijk[:1200] + rng.integers(8, 56, (1200, 3)) / 64.0).astype(F)
    src = mp[rng.permutation(1200)[:m]].astype(np.float64) + rng.normal(0, 0.05, (m, 3)) + [0.03, -0.02, 0.01]
    return reg([(mp, EYE)], src, 1.0, constants=dict(map_capacity=4096))


def cap_iterations(max_iterations):
    """600 map points, their own copies as the source, a guess 1.7 m and 5 degrees off (more than a voxel: the first
    correspondences are wrong ones): the loop runs until |dx| < 1e-4 -- 6 iterations in the restatement -- or until the cap"""
    rng = np.random.default_rng(57)
    ijk, _ = grid(15)
    mp = (ijk[:600] + rng.integers(8, 56, (600, 3)) / 64.0).astype(F)
    return reg([(mp, EYE)], mp, 1.0, rotation_z(5.0, (1.3, 0.9, -0.6)), max_iterations=max_iterations, constants=dict(map_capacity=2048))


REG_CASES = dict({
    "tie_voxels": tie_voxels, "tie_insertion": tie_insertion, "gate_edge": gate_edge,
    "only_27[two away]": lambda: only_27(False), "only_27[adjacent]": lambda: only_27(True), "twentieth_point": twentieth_point,
    "few[2]": lambda: few(2), "few[3]": lambda: few(3), "own_points": own_points},
    **{f"m_seams[{m}]": functools.partial(m_seams, m) for m in M_SEAMS},
    **{"cap_iterations[3]": lambda: cap_iterations(3), "cap_iterations[500]": lambda: cap_iterations(500)})


def restated_registration(case, **wrong):
    """the restatement's answer for a registration case -> (pose, iterations, final |dx|, correspondences); `wrong`:
    find= / gate= of rest.register, to state one wrong decision"""
    if "_arrays" not in case:
        restated_maps(case)
        case["_arrays"] = case["_map"].arrays()
    c = case["constants"]
    return rest.register(case["source"], case["_arrays"], case["guess"], case["sigma"], 1.0, c["max_iterations"],
                         c.get("convergence", 1e-4), fresh=False, **wrong)


# ---- the single wrong decisions a kernel could take, stated through the restatement's own search
def find_last_minimum(map_arrays, x, voxel):
    """the LAST minimum: the search run backwards (voxel offsets reversed, points of a voxel reversed)"""
    keys, counts, pts = map_arrays
    return rest.correspondences((keys, counts, pts[:, ::-1]), x, voxel, rest.OFFSETS[::-1])


OFFSETS_125 = np.concatenate([rest.OFFSETS, np.array([(a, b, c) for a in range(-2, 3) for b in range(-2, 3) for c in range(-2, 3)
                                                      if max(abs(a), abs(b), abs(c)) == 2], dtype=np.int64)])


def find_beyond_27(map_arrays, x, voxel):
    """the 27 voxels, then the shell around them"""
    return rest.correspondences(map_arrays, x, voxel, OFFSETS_125)


def find_19_points(map_arrays, x, voxel):
    """the 20th point of a voxel ignored"""
    keys, counts, pts = map_arrays
    pts = pts.copy()
    pts[:, 19:] = np.inf
    return rest.correspondences((keys, counts, pts), x, voxel)


WRONG = {"last minimum": dict(find=find_last_minimum), "gate <=": dict(gate=np.less_equal), "a 28th voxel": dict(find=find_beyond_27),
         "19 points": dict(find=find_19_points)}
# which wrong decision each case is there to expose (the margin of 1e-3 m / 1e-4 rad is asserted for these)
EXPOSES = {"tie_voxels": ["last minimum"], "tie_insertion": ["last minimum"], "gate_edge": ["gate <="],
           "only_27[two away]": ["a 28th voxel"], "twentieth_point": ["19 points"]}

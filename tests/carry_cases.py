"""The views, poses, pair tables and observation chains the tests of the log tracks share (tests/test_carry.py on the CPU,
tests/test_gpu_carry.py on the GPU).  Not a test module."""
import numpy as np

F = np.float32
SIZES = (0, 1, 2, 512, 513, 2049, 4097)          # the grid's bucket-count steps (H = 2^k >= 2 m) and the seams of its scan tiles
RADIUS = 0.05
NAN_A, NAN_B, NAN_SIGNED = np.array([0x7FC00001, 0x7FC00123, 0xFFC00001], np.uint32).view(F)


def rigid(yaw_deg=0.0, t=(0.0, 0.0, 0.0), pitch_deg=0.0):
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    cp, sp = np.cos(np.radians(pitch_deg)), np.sin(np.radians(pitch_deg))
    P = np.eye(4)
    P[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    P[:3, 3] = t
    return P


POSES = dict(identity=rigid(), yaw30=rigid(30.0, (5.0, -3.0, 0.2)), far=rigid(10.0, (3000.0, -2000.0, 10.0)))     # the last: 3 km out


def views(n, m, seed, pose, radius=RADIUS, ids=50):
    """Two views of one sweep: max(n, m) surface samples around the place the pose carries the origin to; the next view takes n
    of them in an order of its own, the previous view m of them in another, carried back by the inverse pose in float64 and
    stored as float32; a quarter of the next view's rows is pushed up to two radii away, so that hits, misses and rows near
    the radius all occur.  -> (prev float32 [m, 3], prev_id int32 [m], next float32 [n, 3])"""
    rng = np.random.default_rng(seed)
    K = max(n, m)
    base = rng.uniform(-6.0, 6.0, (K, 3)) * np.array([1.0, 1.0, 0.25]) + pose[:3, 3]
    nxt = base[rng.permutation(K)[:n]].copy()
    push = rng.random(n) < 0.25
    nxt[push] += rng.normal(0.0, 1.0, (int(push.sum()), 3)) * radius
    back = base[rng.permutation(K)[:m]] - pose[:3, 3]
    prev = back @ pose[:3, :3]                          # R^T (x - t), row vectors
    return prev.astype(F), rng.integers(-1, ids, m).astype(np.int32), nxt.astype(F)


def at_radius(radius=RADIUS):
    """-> (x_hit, x_miss): the largest float32 x with fl(x * x) <= r2 = fl(fl(r) * fl(r)) and the next float32, found by search"""
    rf = F(radius)
    r2 = rf * rf
    x = rf
    while F(np.nextafter(x, F(np.inf))) * F(np.nextafter(x, F(np.inf))) <= r2:
        x = F(np.nextafter(x, F(np.inf)))
    while x * x > r2:
        x = F(np.nextafter(x, F(-np.inf)))
    return x, F(np.nextafter(x, F(np.inf)))


# ------------------------------------------------------------------------------------------------------------------ the pair ids

def pair_table(P, seed, labels=40, stride=10):
    """P pair rows of `stride` columns over a pool of labels that holds both zeros, NaNs, ground and noise, so that labels are
    shared among pairs; ids with -1 among them; weights with ties among them"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.array([-1e8, -1.0, -0.0, 0.0, np.inf, NAN_A, NAN_B, NAN_SIGNED], F), (np.arange(labels) * 1.5 + 1.0).astype(F)])
    rows = rng.normal(0, 1, (P, stride)).astype(F)
    rows[:, 0], rows[:, 1] = pool[rng.integers(0, len(pool), P)], pool[rng.integers(0, len(pool), P)]
    ids = rng.integers(-1, 4 * labels, P).astype(np.int32)
    weight = rng.integers(0, 4, P).astype(np.float64) * 10.0
    return pool, rows, ids, weight


# ------------------------------------------------------------------------------------------------------------------- the paths

def observation(track, seconds, d, centre=(0.0, 0.0, 0.0), size=(4.0, 2.0, 1.5), points=50):
    return [track, 0.0, seconds, d[0], d[1], d[2], size[0], size[1], size[2], points, centre[0], centre[1], centre[2]]


IDENTITY_FRAME = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]


def three_step_chain():
    """One track at steps 0, 1, 2 in identity frames, s = 0.125: d = (0.25, 0, 0), (0.25, 0.125, 0), (0.5, 0.125, 0), so
    v = (2, 0, 0), (2, 1, 0), (4, 1, 0); the velocity changes by 1 and then by 2; the centres follow the displacements except
    for 0.5 m at the last step.  Every number is exact in binary.  -> (obs, step, frames, the row it must give)"""
    obs = [observation(0, 0.125, (0.25, 0.0, 0.0), centre=(1.0, 2.0, 0.5), points=10),
           observation(0, 0.125, (0.25, 0.125, 0.0), centre=(1.25, 2.0, 0.5), size=(5.0, 1.0, 1.0), points=30),
           observation(0, 0.125, (0.5, 0.125, 0.0), centre=(1.5, 2.625, 0.5), points=20)]
    want = [0, 3, 0, 2, 0, 0.375, 0.25 + np.sqrt(0.25 ** 2 + 0.125 ** 2) + np.sqrt(0.5 ** 2 + 0.125 ** 2), 1.0 / 0.375, 0.25 / 0.375, 0.0,
            np.sqrt((1.0 / 0.375) ** 2 + (0.25 / 0.375) ** 2), 2.0, 2, 0.5, 1, 1, 0, 5.0, 2.0, 1.5, 30, 1.0, 2.0, 0.5]
    return obs, [0, 1, 2], [IDENTITY_FRAME] * 3, want


def random_path_table(seed, T=6, files=5):
    """observations of T tracks over `files` files with rotated frames: missing steps, several observations a step, ids without
    a track, steps outside the files"""
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(files):
        P = rigid(rng.uniform(-180, 180), rng.normal(0, 20, 3), rng.uniform(-5, 5))
        frames.append(np.concatenate([P[:3, :3].reshape(9), P[:3, 3]]))
    obs, step = [], []
    for k in range(files):
        for _ in range(int(rng.integers(0, 2 * T))):
            t = int(rng.integers(-1, T + 1))
            obs.append(observation(t, float(rng.choice([0.1, 0.2])), rng.normal(0, 0.05, 3), rng.normal(0, 30, 3), rng.random(3) * 5, int(rng.integers(1, 4)) * 10))
            step.append(k if rng.random() > 0.05 else int(rng.choice([-1, files])))
    return np.array(obs).reshape(-1, 13), np.array(step, np.int32), np.array(frames).reshape(files, 12), T

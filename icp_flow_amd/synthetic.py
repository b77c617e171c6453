"""Synthetic cluster-pair batches for the measurement harness.

numpy only; deterministic per pair: pair k is generated from
numpy.random.default_rng(seed + k), so any rank can materialise its own shard.
"""
import numpy as np

PAD_VALUE = 1e8


def _shell_points(rng, ext, n):
    """n points uniform on 3 visible faces (front, side, top) of a box of extents ext."""
    lx, ly, lz = ext
    areas = np.array([ly * lz, lx * lz, lx * ly])
    face = rng.choice(3, size=n, p=areas / areas.sum())
    u = rng.uniform(-0.5, 0.5, size=(n, 3)) * ext
    u[face == 0, 0] = 0.5 * lx
    u[face == 1, 1] = 0.5 * ly
    u[face == 2, 2] = 0.5 * lz
    return u


def make_pair(k, n_src, n_dst, max_points, seed=0, noise=0.01):
    """One vehicle-like cluster pair -> (src [N,4], dst [N,4], T_true [4,4]) float32."""
    rng = np.random.default_rng(seed + k)
    ext = np.array([rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.0)])
    centre = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(0.0, 1.5)])
    yaw = np.deg2rad(rng.uniform(-3.0, 3.0))
    t = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(-0.05, 0.05)])
    c, s = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    heading = rng.uniform(-np.pi, np.pi)
    ch, sh = np.cos(heading), np.sin(heading)
    Rh = np.array([[ch, -sh, 0.0], [sh, ch, 0.0], [0.0, 0.0, 1.0]])
    if k % 2 == 0:
        # shared surface samples: the smaller cloud is a subset of the larger one
        shared = _shell_points(rng, ext, max(n_src, n_dst))
        local_src, local_dst = shared[:n_src], shared[:n_dst].copy()
    else:
        local_src = _shell_points(rng, ext, n_src)
        local_dst = _shell_points(rng, ext, n_dst)        # independently resampled surface
    src = local_src @ Rh.T + centre
    dst = (local_dst @ Rh.T) @ Rz.T + centre + t + rng.normal(0.0, noise, size=(n_dst, 3))
    T = np.eye(4)
    T[:3, :3] = Rz
    T[:3, 3] = centre + t - Rz @ centre

    def pad(p):
        out = np.full((max_points, 4), PAD_VALUE, dtype=np.float32)
        out[:, 3] = 0.0
        out[:len(p), 0:3] = p.astype(np.float32)
        out[:len(p), 3] = 1.0
        return out

    return pad(src), pad(dst), T.astype(np.float32)


def make_batch(num_pairs, max_points, seed=0, first=0, ragged=False, n_min=20):
    """[B,N,4] src/dst float32 + ground-truth transforms [B,4,4].

    ragged=False: n_src = n_dst = max_points (BASELINE configs 2 and 4).
    ragged=True : n ~ logUniform(n_min, max_points), padded with (1e8,1e8,1e8,0); the two clouds of a pair draw their
                  sizes independently (a 35-point cluster may face a 7000-point one).
    ragged="matched": n_src as above, n_dst = n_src * U(0.8, 1.25) -- the same object seen from two ranges, which is what
                  the candidate pairs of match_pcds are after sanity_check (similar extents, utils_check.py:21-49).
    """
    S = np.empty((num_pairs, max_points, 4), np.float32)
    D = np.empty((num_pairs, max_points, 4), np.float32)
    T = np.empty((num_pairs, 4, 4), np.float32)
    for i in range(num_pairs):
        k = first + i
        if ragged:
            r = np.random.default_rng(10_000_019 + seed + k)
            ns = int(round(np.exp(r.uniform(np.log(n_min), np.log(max_points)))))
            nd = int(round(np.exp(r.uniform(np.log(n_min), np.log(max_points)))))
            if ragged == "matched":
                nd = int(min(max(round(ns * r.uniform(0.8, 1.25)), n_min), max_points))
        else:
            ns = nd = max_points
        S[i], D[i], T[i] = make_pair(k, ns, nd, max_points, seed)
    return S, D, T


def make_frame_pair(seed=0, n_objects=24, n_min=30, n_max=1500, relabel=0.25, n_background=4000, noise=0.01):
    """A labelled synthetic frame pair in the format of the frame-pair stream (frame_pairs.py).

    n_objects vehicle-like shells on a jittered 14 m grid, object k with n_k ~ logUniform(n_min,
    n_max) source points (the destination frame sees 0.8-1.25x as many of the same surface samples,
    plus sensor noise), each moved by a small
    rigid motion (yaw <= 3 deg, |t_xy| <= 0.8 m).  Source label of object k is k; in the destination
    frame a fraction `relabel` of the objects carries a fresh label (their association has to come
    from stage 2 of match_pcds).  Background: static points labelled ground (-1e8) and noise (-1).
    -> dict(points_src, points_dst, labels_src, labels_dst, pose, gt_flow, T_true [n_objects,4,4])."""
    rng = np.random.default_rng(77_000_003 + seed)
    side = int(np.ceil(np.sqrt(n_objects)))
    ps, pd, ls, ld, gt, Ts = [], [], [], [], [], []
    fresh = 1000
    for k in range(n_objects):
        ns = int(round(np.exp(rng.uniform(np.log(n_min), np.log(n_max)))))
        nd = int(round(ns * rng.uniform(0.8, 1.25)))
        ext = np.array([rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.0)])
        centre = np.array([(k % side - side / 2) * 14.0 + rng.uniform(-2, 2), (k // side - side / 2) * 14.0 + rng.uniform(-2, 2),
                           rng.uniform(0.5, 1.2)])
        yaw = np.deg2rad(rng.uniform(-3.0, 3.0))
        t = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-0.03, 0.03)])
        c, s = np.cos(yaw), np.sin(yaw)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        h = rng.uniform(-np.pi, np.pi)
        Rh = np.array([[np.cos(h), -np.sin(h), 0.0], [np.sin(h), np.cos(h), 0.0], [0.0, 0.0, 1.0]])
        shared = _shell_points(rng, ext, max(ns, nd))     # sparse clusters: both frames see the same samples
        src = shared[:ns] @ Rh.T + centre
        dst = (shared[:nd] @ Rh.T) @ Rz.T + centre + t + rng.normal(0.0, noise, size=(nd, 3))
        T = np.eye(4)
        T[:3, :3] = Rz
        T[:3, 3] = centre + t - Rz @ centre
        ps.append(src); pd.append(dst)
        ls.append(np.full(ns, float(k)))
        moved = rng.uniform() < relabel
        ld.append(np.full(nd, float(fresh if moved else k)))
        fresh += 1 if moved else 0
        gt.append(src @ Rz.T + T[:3, 3] - src)
        Ts.append(T)
    span = side * 7.0 + 10.0
    for lab, frac in ((-1e8, 0.8), (-1.0, 0.2)):
        n = int(n_background * frac)
        bg = np.stack([rng.uniform(-span, span, n), rng.uniform(-span, span, n), rng.uniform(-0.2, 0.1, n)], axis=1)
        ps.append(bg); ls.append(np.full(n, lab)); gt.append(np.zeros((n, 3)))
        pd.append(bg + rng.normal(0.0, noise, size=bg.shape)); ld.append(np.full(n, lab))
    perm_s, perm_d = rng.permutation(sum(map(len, ps))), rng.permutation(sum(map(len, pd)))
    f32 = lambda parts, perm: np.concatenate(parts, axis=0).astype(np.float32)[perm]
    return dict(points_src=f32(ps, perm_s), points_dst=f32(pd, perm_d), labels_src=f32(ls, perm_s),
                labels_dst=f32(ld, perm_d), pose=np.eye(4, dtype=np.float32), gt_flow=f32(gt, perm_s),
                T_true=np.stack(Ts).astype(np.float32))


def make_sequence(seed=0, num_frames=3, n_objects=10, n_min=60, n_max=600, speed=1.2, n_background=1500, noise=0.01):
    """A synthetic multi-frame sample in the reference's Waymo / nuScenes format (dataset_pca.py:41-45): the ego
    vehicle drives along x, `n_objects` vehicle-like shells move with constant velocity (up to `speed` m per frame)
    and yaw rate, static background points are labelled ground.  Frame j is given in ITS OWN ego coordinates
    (raw_points), ego_motion_gt[j] maps them into frame 0's, scene_flow is the reference's ground truth
    (dataset_pca.py:67-69: where the point is at time 0, in frame-0 coordinates, minus the raw point).
    -> dict(raw_points [m,3], time_indice [m], ego_motion_gt [F,4,4], nonground [m], scene_flow [m,3])."""
    rng = np.random.default_rng(55_000_007 + seed)
    side = int(np.ceil(np.sqrt(n_objects)))

    def rz(a):
        c, s_ = np.cos(a), np.sin(a)
        return np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])

    objs = []
    for k in range(n_objects):
        n = int(round(np.exp(rng.uniform(np.log(n_min), np.log(n_max)))))
        ext = np.array([rng.uniform(1.5, 5.0), rng.uniform(1.0, 2.2), rng.uniform(1.0, 2.0)])
        centre = np.array([(k % side - side / 2) * 12.0 + rng.uniform(-2, 2), (k // side - side / 2) * 12.0 + rng.uniform(-2, 2),
                           rng.uniform(0.5, 1.2)])
        heading = rng.uniform(-np.pi, np.pi)
        vel = rng.uniform(0.3, 1.0) * speed * np.array([np.cos(heading), np.sin(heading), 0.0]) * (rng.uniform() < 0.7)
        yaw_rate = np.deg2rad(rng.uniform(-1.5, 1.5))
        objs.append((_shell_points(rng, ext, n) @ rz(heading).T, centre, vel, yaw_rate))
    span = side * 6.0 + 10.0
    bg = np.stack([rng.uniform(-span, span, n_background), rng.uniform(-span, span, n_background),
                   rng.uniform(-0.2, 0.1, n_background)], axis=1)
    ego_v = np.array([rng.uniform(0.5, 1.5), rng.uniform(-0.1, 0.1), 0.0])
    ego_yaw = np.deg2rad(rng.uniform(-0.8, 0.8))
    raw, tim, ng, sf, poses = [], [], [], [], []
    for j in range(num_frames):
        P = np.eye(4)                                        # frame-j ego coordinates -> frame-0 coordinates
        P[:3, :3], P[:3, 3] = rz(ego_yaw * j), ego_v * j
        Pinv = np.linalg.inv(P)
        poses.append(P)
        w0s, wjs, flags = [], [], []
        for local, centre, vel, yaw_rate in objs:
            keep = rng.random(len(local)) < 0.9              # every frame sees most of the same surface samples
            w0 = local[keep] + centre                         # world (= frame 0) position at time 0
            wj = (local[keep] @ rz(yaw_rate * j).T) + centre + vel * j + rng.normal(0.0, noise, size=(int(keep.sum()), 3))
            w0s.append(w0); wjs.append(wj); flags.append(np.ones(len(w0), bool))
        w0s.append(bg); wjs.append(bg + rng.normal(0.0, noise, size=bg.shape)); flags.append(np.zeros(len(bg), bool))
        w0, wj = np.concatenate(w0s), np.concatenate(wjs)
        r = wj @ Pinv[:3, :3].T + Pinv[:3, 3]                 # what the sensor of frame j sees
        perm = rng.permutation(len(r))
        raw.append(r[perm]); tim.append(np.full(len(r), j)); ng.append(np.concatenate(flags)[perm]); sf.append((w0 - r)[perm])
    return dict(raw_points=np.concatenate(raw).astype(np.float32), time_indice=np.concatenate(tim).astype(np.int64),
                ego_motion_gt=np.stack(poses).astype(np.float64), nonground=np.concatenate(ng),
                scene_flow=np.concatenate(sf).astype(np.float32))


# ---- a log: consecutive frame-pair files that share their sweeps ------------------------------------------------------------
LOG_SWEEP_SECONDS = 0.1
LOG_CLUSTER = dict(cluster="dbscan", epsilon=0.25, min_cluster_size=10, num_clusters=200)     # what make_log is made for
# the objects of a log, in the world frame (the sensor frame of sweep 0): centre at sweep 0, metres per sweep, size (a width of
# 0: a wall, one face).  Object LOG_BRAKING loses 3 m/s from file LOG_BRAKE_FILE on; object LOG_LATE is first seen in sweep
# LOG_LATE_FILE (the source of that file); the wall stands.
LOG_CENTRES = np.array([[12.0, 8.0, 0.0], [-10.0, 12.0, 0.0], [14.0, -12.0, 0.0], [-12.0, -10.0, 0.0], [0.0, 20.0, 0.0], [22.0, 0.0, 0.0]])
LOG_STEPS = np.array([[0.4, 0.0, 0.0], [-0.2, 0.3, 0.0], [0.5, 0.0, 0.0], [0.0, -0.35, 0.0], [0.3, 0.1, 0.0], [0.0, 0.0, 0.0]])
LOG_SIZES = np.array([[3.0, 1.6, 1.0], [3.0, 1.6, 1.0], [3.0, 1.6, 1.0], [2.4, 1.4, 1.0], [3.0, 1.6, 1.0], [6.0, 0.0, 1.0]])
LOG_BRAKING, LOG_BRAKE_FILE, LOG_BRAKE_LOSS = 2, 3, np.array([0.3, 0.0, 0.0])       # 0.3 m per 0.1 s sweep: 3 m/s
LOG_LATE, LOG_LATE_FILE, LOG_WALL = 4, 2, 5


def _box_faces(rng, size, spacing=0.1, jitter=0.03):
    """points on the four vertical faces of a box (a wall: one face), a jittered grid: every point has neighbours within
    spacing + 2 jitter along its face"""
    L, W, H = size
    corners = [(-L / 2, -W / 2), (L / 2, -W / 2), (L / 2, W / 2), (-L / 2, W / 2)]
    edges = [(corners[k], corners[(k + 1) % 4]) for k in range(4)] if W > 0 else [((-L / 2, 0.0), (L / 2, 0.0))]
    pts = []
    for (x0, y0), (x1, y1) in edges:
        steps = int(round(np.hypot(x1 - x0, y1 - y0) / spacing))
        for a in (np.arange(steps) + 0.5) / steps:
            for z in np.arange(-H / 2 + spacing / 2, H / 2, spacing):
                pts.append((x0 + a * (x1 - x0), y0 + a * (y1 - y0), z))
    pts = np.array(pts)
    return pts + rng.uniform(-jitter, jitter, pts.shape)


def log_centre(k, sweep):
    """the world position of object k's centre at `sweep`: its step per sweep, less what the braking object loses per sweep from
    sweep LOG_BRAKE_FILE on"""
    late = max(sweep - LOG_BRAKE_FILE, 0) if k == LOG_BRAKING else 0
    return LOG_CENTRES[k] + sweep * LOG_STEPS[k] - late * LOG_BRAKE_LOSS


def make_log(seed=0, files=6, ego_speed=8.0, ego_yaw_rate_deg=15.0, drop=0.1, noise=0.005, ground_spacing=1.0, extra=0):
    """A log of `files` consecutive frame-pair files for unlabelled use with LOG_CLUSTER: file k registers sweep k onto sweep
    k + 1.  An ego vehicle at `ego_speed` m/s with a yaw rate; boxes at constant velocity, one that loses 3 m/s between two
    files, one that appears in file LOG_LATE_FILE, a static wall, and ground (flagged, as ground removal upstream leaves it).
    Every sweep is sampled ONCE, in its own sensor frame; its two views -- the destination of file k - 1 and the source of file
    k -- are made differently: each is shuffled by a permutation of its own, each drops `drop` of the rows independently, they
    are cropped differently (the destination to a square of 30 m, the source to a circle of 33 m), and the source view is
    stored as the float32 of the float64 product with the file's pose, which carries sweep k's frame into sweep k + 1's.
    extra (the timing tool's; the tests leave it 0): that many more boxes at up to 1.5 m/s on the free cells of a 7.5 m grid;
    ground_spacing sets the rows of a sweep.
    -> (pairs, truth): pairs a list of dicts(points_src, points_dst, pose, nonground_src, nonground_dst), what
    pair_data.FramePair takes; truth dict(ids_src, ids_dst: per file the object of every row, -1 for ground, -2 for a few isolated points; velocity float64
    [objects, files, 3]: every object's true velocity over file k in the LOG's frame, the destination frame of file 0; seen
    bool [objects, files])"""
    rng = np.random.default_rng(77_000_003 + seed)
    dt = LOG_SWEEP_SECONDS
    shapes = [_box_faces(rng, s) for s in LOG_SIZES]
    more = []                                              # (centre, step) of the extra boxes
    if extra:
        cells = [(x, y) for x in np.arange(-26.0, 27.0, 7.5) for y in np.arange(-26.0, 27.0, 7.5)
                 if min(np.hypot(x - log_centre(j, k)[0], y - log_centre(j, k)[1]) for j in range(len(LOG_SIZES)) for k in (0, files)) > 7.0]
        for x, y in [cells[i] for i in rng.permutation(len(cells))[:extra]]:
            more.append((np.array([x, y, 0.0]), np.append(rng.uniform(-0.15, 0.15, 2), 0.0)))
            shapes.append(_box_faces(rng, np.array([rng.uniform(2.0, 3.0), rng.uniform(1.2, 1.8), 1.0])))
    span = 34.0
    axis = np.arange(-span, span + 1e-9, ground_spacing)
    gx, gy = np.meshgrid(axis, axis, indexing="ij")

    def rz(a):
        c, s_ = np.cos(a), np.sin(a)
        return np.array([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])

    ego = []                                               # sensor frame of sweep k -> world
    at, yaw = np.zeros(3), 0.0
    for k in range(files + 1):
        E = np.eye(4)
        E[:3, :3], E[:3, 3] = rz(yaw), at
        ego.append(E)
        yaw += np.radians(ego_yaw_rate_deg) * dt
        at = at + rz(yaw) @ np.array([ego_speed * dt, 0.0, 0.0])
    sweeps = []
    for k in range(files + 1):
        pts, obj = [], []
        for j, local in enumerate(shapes):
            if j == LOG_LATE and k < LOG_LATE_FILE:
                continue
            centre = log_centre(j, k) if j < len(LOG_SIZES) else more[j - len(LOG_SIZES)][0] + k * more[j - len(LOG_SIZES)][1]
            world = local + centre + np.array([0.0, 0.0, 0.8]) + rng.normal(0.0, noise, local.shape)
            pts.append((world - ego[k][:3, 3]) @ ego[k][:3, :3])          # R^T (x - t), row vectors
            obj.append(np.full(len(local), j))
        ground = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(gx.size)], axis=1) + rng.uniform(-0.3, 0.3, (gx.size, 3)) * np.array([1.0, 1.0, 0.05])
        pts.append(ground), obj.append(np.full(len(ground), -1))
        # a few isolated points as noise (the reference's keep_largest drops the first label unseen, which is the noise label only
        # when there is noise)
        lonely = np.stack([np.linspace(-12.0, 12.0, 6), np.full(6, 27.0), np.full(6, 0.5)], axis=1) + rng.uniform(-0.2, 0.2, (6, 3))
        pts.append(lonely), obj.append(np.full(6, -2))
        sweeps.append((np.concatenate(pts), np.concatenate(obj)))

    def view(points, obj, keep):
        rows = np.flatnonzero(keep)
        rows = rows[rng.permutation(len(rows))]
        rows = rows[: len(rows) - int(round(drop * len(rows)))]
        return points[rows], obj[rows]

    pairs, ids_src, ids_dst = [], [], []
    for k in range(files):
        pose = np.linalg.inv(ego[k + 1]) @ ego[k]
        p, o = sweeps[k]
        src, src_obj = view(p, o, np.hypot(p[:, 0], p[:, 1]) < 33.0)
        src = (src @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)     # the float64 product, then narrowed
        p, o = sweeps[k + 1]
        dst, dst_obj = view(p, o, (np.abs(p[:, 0]) < 30.0) & (np.abs(p[:, 1]) < 30.0))
        pairs.append(dict(points_src=src, points_dst=dst.astype(np.float32), pose=pose, nonground_src=src_obj != -1, nonground_dst=dst_obj != -1))
        ids_src.append(src_obj), ids_dst.append(dst_obj)
    to_log = ego[1][:3, :3].T                                # world -> the destination frame of file 0
    velocity = np.array([[to_log @ ((log_centre(j, k + 1) - log_centre(j, k)) / dt) for k in range(files)] for j in range(len(LOG_SIZES))]
                        + [[to_log @ (step / dt)] * files for _, step in more])
    seen = np.array([[not (j == LOG_LATE and k < LOG_LATE_FILE) for k in range(files)] for j in range(len(shapes))])
    return pairs, dict(ids_src=ids_src, ids_dst=ids_dst, velocity=velocity, seen=seen)

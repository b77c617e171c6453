"""The labellings, chains and motions the tests of the object tracks share (tests/test_tracks.py on the CPU,
tests/test_gpu_tracks.py on the GPU).  Not a test module."""
import numpy as np

F = np.float32
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
NAN_A, NAN_B, NAN_SIGNED = np.array([0x7FC00001, 0x7FC00123, 0xFFC00001], np.uint32).view(F)
SPECIAL = np.array([-1e8, -1.0, -np.inf, -0.0, 0.0, 2.5, 1e7, np.inf, NAN_A, NAN_B, NAN_SIGNED], F)


def random_pair(n, seed, labels_a=7, labels_b=5):
    """two labellings of n rows: a few clusters a side, ground and noise among them"""
    rng = np.random.default_rng(seed)
    pool = lambda k: np.concatenate([[-1e8, -1.0], np.arange(k, dtype=np.float64) * 1.5]).astype(F)   # noqa: E731
    return rng.choice(pool(labels_a), n).astype(F), rng.choice(pool(labels_b), n).astype(F)


def long_segment(cuts):
    """one segment of 2049 rows (three chunks of 1024 rows of the stable order) split over three partner segments at `cuts`,
    between 300 rows of another cluster and 200 of ground that both sides share"""
    a = np.concatenate([np.full(300, 2.0), np.full(2049, 5.0), np.full(200, -1e8)]).astype(F)
    b = np.concatenate([np.full(300, 9.0), np.repeat([1.0, 2.0, 3.0], [cuts[0], cuts[1] - cuts[0], 2049 - cuts[1]]), np.full(200, -1e8)]).astype(F)
    return a, b


LONG_CUTS = ((700, 1500), (1024, 2048), (1023, 1025), (1, 2048))     # inside the chunks, on both seams, one row either side


def many_segments():
    """4096 segments a side at n = 8192, every segment of one side across two of the other"""
    i = np.arange(8192)
    return (i // 2).astype(F), (((i + 1) // 2) % 4096).astype(F)


def special_labels(seed=3):
    rng = np.random.default_rng(seed)
    return SPECIAL[rng.integers(0, len(SPECIAL), 400)], SPECIAL[rng.integers(0, len(SPECIAL), 400)]


def tie_two_two():
    """segment 7 of A meets segments 1 and 2 of B in two rows each: the partner is the lower one"""
    return np.array([7, 7, 7, 7, 3], F), np.array([2, 1, 1, 2, 2], F)


def tie_mutual():
    """X = {0, 1}, Y = {2, 3} against P = {0, 2}, Q = {1, 3}: every intersection is one row, every partner a tie -- X and P take
    each other, Y and Q both point at a segment that points elsewhere; with ties to the HIGHER index Y and Q would be mutual"""
    return np.array([10, 10, 20, 20], F), np.array([1, 2, 1, 2], F)


def all_negative_other_side():
    return np.array([3, 3, 3, 4, 4, -1], F), np.array([-1, -1e8, -np.inf, 6, 6, 6], F)


def relabelled(n=500, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 9, n).astype(F)
    perm = rng.permutation(9).astype(F)
    return a, perm[a.astype(np.int64)]


# ---------------------------------------------------------------------------------------------------------------- the chain

def _rows(n, **sets):
    lab = np.full(n, -1.0, F)
    for value, rows in sets.values():
        lab[list(rows)] = value
    return lab


CHAIN_ROWS = 30


def chain():
    """Three gaps over 30 rows, and what every gap must give.  Gap 1 founds tracks 0-5 (ascending label order).  Gap 2: A
    unchanged under a new label inherits 0; B = rows 6-11 splits into 6-9 (IoU 4/6, inherits 1) and 10-11 (its partner, track 1,
    points at the larger part: fresh, id 6); C (12-14) and D (15-18) merge: the partner is D (4 rows of 7, IoU 4/7, inherits 3),
    track 2 is seen by no segment; E (19-21) is unseen (its rows are noise) and keeps id 4 on its rows; G (22-24) unchanged.
    Gap 3: E comes back and inherits 4; a cluster of rows 23-25 meets G in 2 rows of 3 + 3 - 2: IoU exactly 1/2 = min_iou,
    inherits 5 (fresh above min_iou); everything else noise."""
    g1 = _rows(CHAIN_ROWS, A=(10.0, range(0, 6)), B=(20.0, range(6, 12)), C=(30.0, range(12, 15)), D=(40.0, range(15, 19)),
               E=(50.0, range(19, 22)), G=(60.0, range(22, 25)))
    g2 = _rows(CHAIN_ROWS, A=(7.0, range(0, 6)), B1=(8.0, range(6, 10)), B2=(9.0, range(10, 12)), CD=(11.0, range(12, 19)), G=(12.0, range(22, 25)))
    g3 = _rows(CHAIN_ROWS, E=(1.0, range(19, 22)), G=(2.0, range(23, 26)))
    ids1 = np.full(CHAIN_ROWS, -1, np.int32)
    for t, rows in enumerate((range(0, 6), range(6, 12), range(12, 15), range(15, 19), range(19, 22), range(22, 25))):
        ids1[list(rows)] = t
    ids2 = ids1.copy()
    ids2[10:12] = 6
    ids2[12:15] = 3
    ids3 = ids2.copy()
    ids3[25] = 5
    return [dict(labels=g1, ids=ids1, next_id=6, segment_ids=[-1, 0, 1, 2, 3, 4, 5], inherited=[0, 0, 0, 0, 0, 0, 0]),
            dict(labels=g2, ids=ids2, next_id=7, segment_ids=[-1, 0, 1, 6, 3, 5], inherited=[0, 1, 1, 0, 1, 1]),
            dict(labels=g3, ids=ids3, next_id=7, segment_ids=[-1, 4, 5], inherited=[0, 1, 1])]


# ---------------------------------------------------------------------------------------------------------------- the scene

SCENE_FRAMES, SCENE_SWEEP_SECONDS = 4, 0.1
SCENE_CLUSTER = dict(cluster="dbscan", epsilon=0.25, min_cluster_size=10, num_clusters=200)
# metres per frame; frame j sees an object at centre + j * step, frame 0 at its centre: the registration of gap j moves it by
# d_j = -j * step, so the truth of the fitted velocity is -step / SCENE_SWEEP_SECONDS
SCENE_STEPS = np.array([[0.4, 0.0, 0.0], [-0.2, 0.3, 0.0], [0.0, -0.45, 0.0], [0.3, 0.1, 0.0], [0.0, 0.0, 0.0]])
SCENE_CENTRES = np.array([[-15.0, -15.0, 0.8], [15.0, -15.0, 0.8], [-15.0, 15.0, 0.8], [15.0, 15.0, 0.8], [0.0, 0.0, 0.8]])
SCENE_SIZES = np.array([[3.0, 1.6, 1.0], [3.0, 1.6, 1.0], [2.4, 1.4, 1.0], [3.0, 1.6, 1.0], [6.0, 0.0, 1.0]])    # the last: a wall
SCENE_BAD, SCENE_BAD_FRAME, SCENE_BAD_OFFSET = 3, 3, np.array([-0.316, 0.949, 0.0])        # 1 m off its line in the last frame
SCENE_WALL = 4


def _faces(rng, size, spacing=0.1, jitter=0.03):
    """points on the four vertical faces of a box (a wall: one face), a jittered grid -- every point has neighbours within
    spacing + 2 jitter along its face, and no two frames' grids alias"""
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


def scene(seed=7, noise=0.005):
    """A 4-frame sample in load_sequence's format, identity ego poses: three rigid boxes at constant velocity, one whose third
    displacement is 1 m off its line, a static wall, and a few isolated points as noise (the reference's keep_largest drops the
    first label unseen, which is the noise label only when there is noise).  -> dict(arrays = the file's keys, object [m] = the
    object of every row, -1 for noise)"""
    rng = np.random.default_rng(seed)
    shapes = [_faces(rng, s) for s in SCENE_SIZES]
    raw, tim, obj = [], [], []
    for j in range(SCENE_FRAMES):
        for k, local in enumerate(shapes):
            at = SCENE_CENTRES[k] + j * SCENE_STEPS[k] + (SCENE_BAD_OFFSET if (k == SCENE_BAD and j == SCENE_BAD_FRAME) else 0.0)
            raw.append(local + at + rng.normal(0.0, noise, local.shape))
            obj.append(np.full(len(local), k))
        lonely = np.stack([np.linspace(-30, 30, 6), np.full(6, 30.0 + j), np.full(6, 0.5)], axis=1)
        raw.append(lonely)
        obj.append(np.full(6, -1))
        tim.append(np.full(sum(len(s) for s in shapes) + 6, j))
    arrays = dict(raw_points=np.concatenate(raw).astype(F), time_indice=np.concatenate(tim).astype(np.int64),
                  ego_motion=np.tile(np.eye(4), (SCENE_FRAMES, 1, 1)))
    return dict(arrays=arrays, object=np.concatenate(obj))


def scene_truth_velocity():
    return -SCENE_STEPS / SCENE_SWEEP_SECONDS


def object_row(label_dst, d=(0.0, 0.0, 0.0), size=(4.0, 2.0, 1.5), points=50, centre=(10.0, 5.0, 1.0), label_src=3.0):
    """one row of icpflow_pair_objects' table with what the observations read (tests/box_restatement.pair_objects's columns)"""
    row = np.zeros(24)
    row[0:2] = label_src, label_dst
    row[4:7], row[7:10], row[16:19], row[22] = centre, d, size, points
    return row


def observation(track, gap, seconds, d, size=(4.0, 2.0, 1.5), points=50):
    return [track, gap, seconds, d[0], d[1], d[2], size[0], size[1], size[2], points, 0.0, 0.0, 0.0]

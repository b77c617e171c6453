"""The inputs of tests/test_gpu_match_eval.py (NumPy only), the path each is built for -- the host's decisions and the kernel's
predicates restated from csrc/api.hip (eval_by_sweep, Workspace::shareScratch) and csrc/nn.hip (scan_queries_per_lane, launch_sweep,
sweep_job) --, and the geometric conditions that make a case the case its name claims, so that tests/test_match_eval_restatement.py
can check all of it on the CPU.  Batches [B, N, 4] float32 in the pad_segment layout (valid rows first, w = 1; pads
(1e8, 1e8, 1e8, 0) behind them).  The restated results are cached per case here (`restated`).  Not a test module."""
import numpy as np

import match_eval_restatement as mr
import sort_cases as sc
import sort_restatement as sr

F = np.float32

# ------------------------------------------------------------------------------------------------ the host's decisions
MAX_SORT_N = 16384            # api.hip kMaxSortN
SCORE_SWEEP_MIN_N = 2048      # api.hip kScoreSweepMinN
SCAN_BLOCK = SWEEP_BLOCK = 256
SCAN_TILE, CHUNK, WAVE = 1024, 16, 64
SHARE_SLOTS = 16              # kernels.hpp kSweepShareSlots
FULLSCAN_MIN_N = 2048         # nn.hip kSweepFullScanMinTargets: the padded width from which jobs may be shared
FULL_QB, FULL_MIN_NT, SHARES = 2, 512, 8
SHARE_MIN_TARGETS = 512
STAGE = 4096
R0 = F(0.15)


def eval_by_sweep(B, N, no_eval_sweep=False):
    if N > MAX_SORT_N or no_eval_sweep:
        return False
    return N > SCORE_SWEEP_MIN_N or (N >= 1024 and B * N >= (1 << 18))


def scan_queries_per_lane(N, B):
    return 1 if N <= 512 else (2 if (N <= 1024 or B <= 128) else 4)


def share_scratch(B, N):
    return N >= 2048 and B * 12 * SHARE_SLOTS * 256 * 4 <= (64 << 20)


def share_instantiation(B, N):
    """launch_sweep: sweep_scan_kernel<SWEEP_EVAL, true>"""
    return N >= FULLSCAN_MIN_N and 2 * B <= 12 * 700


def direction_path(nq, nt, B, N):
    """One direction of one pair in the sweep launch -> (token, shares, staged): 'empty' (no query or no target), 'full' (fullScan),
    'shared' (the LAST block is a sharedWindow; the blocks before it plain windows), 'window'"""
    share = share_instantiation(B, N)
    counters = share and share_scratch(B, N)                       # p.shareCount != nullptr
    qblocks, nqb = -(-N // SWEEP_BLOCK), -(-nq // SWEEP_BLOCK)
    staged = -(-nt // CHUNK) * CHUNK <= STAGE
    if nq == 0 or nt == 0:
        return "empty", 1, staged
    if counters and nqb <= FULL_QB and nt >= FULL_MIN_NT and qblocks >= 2 * nqb:
        return "full", min(qblocks // nqb, SHARES), staged
    if share and nq - (nqb - 1) * SWEEP_BLOCK <= WAVE and nt >= SHARE_MIN_TARGETS:
        return "shared", 1, staged
    return "window", 1, staged


def paths(case, no_eval_sweep=False):
    """-> dict(kernel: 'scan<Q>' | 'sweep<plain>' | 'sweep<SHARE>', dirs: [B][2] of direction_path's tuples (sweeps only))"""
    B, N = case["P1"].shape[:2]
    if not eval_by_sweep(B, N, no_eval_sweep):
        return dict(kernel=f"scan<{scan_queries_per_lane(N, B)}>", dirs=None)
    lens = [(mr.length(a), mr.length(c)) for a, c in zip(case["P1"], case["P2"])]
    return dict(kernel="sweep<SHARE>" if share_instantiation(B, N) else "sweep<plain>",
                dirs=[[direction_path(n1, n2, B, N), direction_path(n2, n1, B, N)] for n1, n2 in lens])


def tokens(p):
    return set() if p["dirs"] is None else {f"{t}{s if t == 'full' else ''}" for d in p["dirs"] for t, s, _ in d}


# ------------------------------------------------------------------------------------------------ building blocks
def pose(yaw=0.0, t=(0.0, 0.0, 0.0), scale=1.0, reflect=False):
    c, s = np.cos(yaw), np.sin(yaw)
    M = np.eye(4)
    M[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) * scale
    if reflect:
        M[:3, 1] = -M[:3, 1]
    M[:3, 3] = t
    return M.astype(F)


def carried_back(points, M):
    """rows that the pose M carries (to rounding) onto `points`"""
    M = np.asarray(M, np.float64)
    return ((np.asarray(points, np.float64) - M[:3, 3]) @ np.linalg.inv(M[:3, :3]).T).astype(F)


def near_pair(rng, n1, n2, M, centre=None, ext=None):
    """pcd2: n2 rows on a vehicle-sized shell; pcd1: n1 rows of the same shell carried back through M"""
    ext = [rng.uniform(2.5, 5), rng.uniform(1.2, 2.2), rng.uniform(1, 2)] if ext is None else ext
    centre = np.array([rng.uniform(-40, 40), rng.uniform(-40, 40), 0.8]) if centre is None else np.asarray(centre, float)
    return carried_back(sc.shell(rng, n1, centre, ext), M), sc.shell(rng, n2, centre, ext)


def sort_code(p1, p2, dir_keys=False):
    """the key code of the pair's sort as the standalone call makes it: pcd2 the fixed cloud, coordinates only (match_eval_core sorts
    on a scratch whose dirKeys nobody set); dir_keys=True: what hist_icp's sort, which icpflow_hist_icp_eval reuses, may choose"""
    n1, n2 = mr.length(p1), mr.length(p2)
    return sr.choose_code(np.asarray(p2, F)[:n2, :3], n1, dir_keys)[0]


def sorted_rows(p1, p2):
    """-> (code, rows of pcd1 in sorted order, rows of pcd2 in sorted order)"""
    code = sort_code(p1, p2)
    n1, n2 = mr.length(p1), mr.length(p2)
    return code, sr.order(sr.axis_key(code, p1[:n1, :3])), sr.order(sr.axis_key(code, p2[:n2, :3]))


def threshold_rows(a, c, M, thres):
    """Four isolated rows appended to each cloud of a pair (a, c: [n, 3]; M with M[2] = (0, 0, 1, 0), so that a moved z is the raw z):
    beyond either end of pcd2 along x, one couple of rows whose distance is EXACTLY float32(thres) -- not an inlier -- and one a
    float32 step inside it -- an inlier; the couples are each other's nearest neighbours, so both directions have both rows.
    The low end's rows go in front of the clouds, the high end's behind them.  -> a', c', (rows of pcd1, rows of pcd2, wanted d)"""
    th = F(thres)
    lo, hi = c[:, 0].min(), c[:, 0].max()
    cy = F(0.5) * (c[:, 1].min() + c[:, 1].max())
    want = [th, np.nextafter(th, F(0)), th, np.nextafter(th, F(0))]
    xs = [lo - F(3.5), lo - F(2.0), hi + F(2.0), hi + F(3.5)]
    A, C = [], []
    for x, w in zip(xs, want):
        hit = None
        for k in range(0, 64):                                   # the float32 z nearest to w whose chain gives w back
            for z in (w,) if k == 0 else (_step(w, k), _step(w, -k)):
                row = carried_back([[x, cy, 0.0]], M)[0]
                row[2] = z
                m = mr.moved(row[None], M)[0]
                tgt = np.array([m[0], m[1], 0.0], F)
                if m[2] == z and np.sqrt(mr.sqdist(m, tgt)) == w:
                    hit = (row, tgt)
                    break
            if hit:
                break
        assert hit is not None, (x, w)
        A.append(hit[0]); C.append(hit[1])
    a2 = np.concatenate([np.array(A[:2], F), a, np.array(A[2:], F)])
    c2 = np.concatenate([np.array(C[:2], F), c, np.array(C[2:], F)])
    return a2, c2, ([0, 1, len(a2) - 2, len(a2) - 1], [0, 1, len(c2) - 2, len(c2) - 1], want)


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def make(pairs, poses, N, thres=0.1, **extra):
    P1, P2 = sc.batch(pairs, N)
    T = np.stack([np.asarray(M, F) for M in poses])
    assert len(T) == len(P1)
    return dict(P1=P1, P2=P2, T=T, thres=thres, **extra)


def cycle_poses(B, rng):
    base = [pose(0.3, (1.5, -0.7, 0.2)), pose(), pose(np.deg2rad(179.9), (0.4, 0.1, -0.1)), pose(-1.1, (-2.0, 0.3, 0.05))]
    return [base[b % 4] for b in range(B)]


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}          # name -> dict(build, kernel, has, conditions)


def case(name, kernel, has=()):
    def deco(fn):
        CASES[name] = dict(build=fn, kernel=kernel, has=set(has))
        return fn
    return deco


def _scan_q1(N):
    def build():
        rng = np.random.default_rng(100 + N)
        lens = [(N, N), (N, max(1, N // 2 + 1)), (max(1, N // 3), N)]
        Ts = cycle_poses(3, rng)
        return make([near_pair(rng, a, c, M) for (a, c), M in zip(lens, Ts)], Ts, N)
    return build


for _n in (1, 16, 17, 256, 257, 512):
    case(f"scan_q1_N{_n}", "scan<1>")(_scan_q1(_n))


def _scan_q2(N):
    def build():
        rng = np.random.default_rng(200 + N)
        Ts = cycle_poses(2, rng)
        return make([near_pair(rng, N, N, Ts[0]), near_pair(rng, 17, N, Ts[1])], Ts, N)
    return build


for _n in (513, 1024, 1025, 2048):          # 1025: ONE row in the last tile; 2048: two full tiles
    case(f"scan_q2_N{_n}", "scan<2>")(_scan_q2(_n))


def ragged_rest(rng, count, Ts, lo=1, hi=20):
    return [near_pair(rng, int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)), M) for M in Ts[-count:]]


@case("scan_q4_B129_N1025", "scan<4>")
def _scan_q4():
    rng = np.random.default_rng(300)
    Ts = cycle_poses(129, rng)
    long = [near_pair(rng, a, c, M) for (a, c), M in zip([(1025, 1025), (1025, 1), (17, 1024)], Ts)]
    return make(long + ragged_rest(rng, 126, Ts), Ts, 1025)


@case("scan_N16385", "scan<2>")
def _scan_beyond_sorts():
    rng = np.random.default_rng(301)
    M = pose(0.3, (1.5, -0.7, 0.2))
    return make([near_pair(rng, 16385, 40, M, ext=(12.0, 6.0, 3.0))], [M], 16385)


@case("sweep_plain_B256_N1024", "sweep<plain>", {"window"})
def _sweep_plain():
    rng = np.random.default_rng(400)
    Ts = cycle_poses(256, rng)
    long = [near_pair(rng, a, c, M) for (a, c), M in zip([(1024, 1024), (1024, 300), (200, 1000), (700, 650)], Ts)]
    return make(long + ragged_rest(rng, 252, Ts, hi=5), Ts, 1024)


def _sweep_share(B):
    def build():
        rng = np.random.default_rng(410 + B)
        Ts = cycle_poses(B, rng)
        lens = [(2049, 2049), (40, 2049), (2049, 300), (900, 700)][:B]
        return make([near_pair(rng, a, c, M) for (a, c), M in zip(lens, Ts)], Ts, 2049)
    return build


for _b, _has in ((1, {"shared"}), (2, {"shared", "full8"}), (3, {"shared", "full8", "full4"}), (4, {"shared", "full8", "full4", "window"})):
    case(f"sweep_share_B{_b}_N2049", "sweep<SHARE>", _has)(_sweep_share(_b))


@case("sweep_share_B128_N2048", "sweep<SHARE>", {"window"})
def _sweep_share_128():
    rng = np.random.default_rng(420)
    Ts = cycle_poses(128, rng)
    long = [near_pair(rng, a, c, M) for (a, c), M in zip([(2048, 1500), (600, 2048)], Ts)]
    return make(long + ragged_rest(rng, 126, Ts, hi=6), Ts, 2048)


@case("sweep_nt_1_15_16_17", "sweep<SHARE>", {"window"})
def _sweep_nt():
    rng = np.random.default_rng(430)
    Ts = cycle_poses(4, rng)
    return make([near_pair(rng, 300, nt, M) for nt, M in zip((1, 15, 16, 17), Ts)], Ts, 2049)


def lattice(nx, ny, nz, step, origin):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g * step + np.asarray(origin)).astype(F)


@case("sweep_rounds", "sweep<SHARE>", {"window"})
def _sweep_rounds():
    """pair 0: dense, settled in round one; 1: a 0.5 m lattice against itself shifted by 0.25 m in y (second round); 2: two clouds
    40 m apart along x under the identity (the radius quadruples until everything is scanned); 3: one wave of 63 near queries and
    one about 4 m off in y"""
    rng = np.random.default_rng(440)
    I = pose()
    dense = near_pair(rng, 900, 900, I, centre=(5.0, 5.0, 0.8), ext=(1.0, 0.5, 0.5))
    lat = (lattice(20, 10, 3, 0.5, (-12.0, 7.0, 0.0)), lattice(20, 10, 3, 0.5, (-12.0, 7.25, 0.0)))
    far = (sc.shell(rng, 600, (-20.0, 3.0, 0.8), (4.0, 2.0, 1.5)), sc.shell(rng, 600, (20.0, 3.0, 0.8), (4.0, 2.0, 1.5)))
    a, c = near_pair(rng, 64, 500, I, centre=(30.0, -10.0, 0.8), ext=(4.0, 1.5, 1.5))
    a = c[rng.choice(500, 64, replace=False)] + F(0.01)           # every query within 2 cm of a target ...
    a[np.argsort(a[:, 0])[32]] += np.array([0.0, 5.0, 0.0], F)    # ... but one
    return make([dense, lat, far, (a, c)], [I] * 4, 2049)


@case("sweep_shared_window", "sweep<SHARE>", {"shared", "window", "full4"})
def _sweep_shared_window():
    rng = np.random.default_rng(450)
    lens = [(n1, n2) for n1 in (513, 576, 577) for n2 in (511, 512, 2049)]
    Ts = cycle_poses(len(lens), rng)
    return make([near_pair(rng, a, c, M) for (a, c), M in zip(lens, Ts)], Ts, 2049)


@case("sweep_fullscan", "sweep<SHARE>", {"full8", "full4", "window"})
def _sweep_fullscan():
    rng = np.random.default_rng(460)
    lens = [(n1, n2) for n1 in (40, 300) for n2 in (512, 513, 2049)]
    lens = lens + [(c, a) for a, c in lens] + [(40, 511), (511, 40)]          # the roles exchanged; 511 targets: the negative
    Ts = cycle_poses(len(lens), rng)
    pairs = []
    for (n1, n2), M in zip(lens, Ts):
        # the LAST target of either direction's sorted order -- alone in the last chunk of 513 or 2049 targets -- is the nearest
        # neighbour of a query 1 mm from it: row 0 of the other cloud (every pair is sorted along x: the shells are longest there)
        a, c = near_pair(rng, n1, n2, M)
        off = np.array([-0.001, 0.001, 0.001], F)                 # (short of the last row along x: the last row stays the last)
        last = lambda p: len(p) - 1 - int(np.argmax(p[::-1, 0]))     # noqa: E731  (stable order: of equal keys the last row)
        a[0] = carried_back(c[last(c)] + off, M)
        c[0] = mr.moved(a[last(a)][None], M)[0] + off
        pairs.append((a, c))
    return make(pairs, Ts, 2049)


@case("sweep_scale_0.95_window", "sweep<SHARE>", {"window"})
def _sweep_shrinking_pose():
    """A pose that SHRINKS (scale 0.95: the backward direction must fall back to the whole cloud).  The window arithmetic puts the
    query c at M^T c = 0.95 c on the key axis while the rows of pcd1 lie at their raw x / 0.95.  The last row of pcd2, alone at
    x = 0.5, has a moved row 0.12 m ahead of it along x -- at 0.653 on the key axis, outside the window that ends at
    0.475 + 0.15 + slack -- and one 0.14 m beside it, at 0.526: inside the window and inside the radius 0.15 * 0.9995 that would end
    the search.  The nearer row opens a chunk of its own (rank 704)."""
    rng = np.random.default_rng(465)
    M = pose(0.0, (0.0, 0.0, 0.0), scale=0.95)
    centre, ext = (-0.7, 5.0, 0.8), (1.0, 0.5, 0.5)
    c0 = np.array([0.5, 5.0, 0.8])
    mv = np.concatenate([sc.shell(rng, 703, centre, ext), [c0 + [0.0, 0.14, 0.0]], [c0 + [0.12, 0.0, 0.0]]])
    c = np.concatenate([sc.shell(rng, 700, centre, ext), [c0]]).astype(F)
    return make([(carried_back(mv, M), c)], [M], 2049)


@case("sweep_staging_N4112", "sweep<SHARE>", {"window"})
def _sweep_staging():
    rng = np.random.default_rng(470)
    lens = [(600, 4096), (600, 4097), (4096, 600), (4097, 600)]
    Ts = cycle_poses(4, rng)
    return make([near_pair(rng, a, c, M, ext=(8.0, 3.0, 2.0)) for (a, c), M in zip(lens, Ts)], Ts, 4112)


@case("sweep_thin_box_45", "sweep<SHARE>", {"window"})
def _sweep_thin_box():
    """sort_cases' thin box turned by 45 degrees, as the fixed cloud and as the moving one: the standalone call sorts it along a
    coordinate; hist_icp's sort, which icpflow_hist_icp_eval reuses, along direction 4"""
    Ts = [pose(0.0, (0.05, -0.03, 0.0)), pose(0.3, (1.5, -0.7, 0.0))]
    pairs = [(carried_back(sc.thin_box(600, 45.0, seed=1), Ts[0]), sc.thin_box(1025, 45.0, seed=2)),
             (carried_back(sc.thin_box(1100, 45.0, seed=3), Ts[1]), sc.thin_box(1030, 45.0, seed=4))]
    return make(pairs, Ts, 2049)


FAR = (3000.0, -2000.0, 0.0)


def pose_list():
    return [("identity", pose()), ("yaw_0.3", pose(0.3, (1.5, -0.7, 0.2))), ("yaw_179.9", pose(np.deg2rad(179.9), (0.4, 0.1, -0.1))),
            ("reflection", pose(0.7, (0.5, 0.2, 0.0), reflect=True)), ("scale_1.05", pose(0.2, (0.3, 0.0, 0.0), scale=1.05)),
            ("scale_1.00004", pose(0.2, (0.3, 0.0, 0.0), scale=1.00004)), ("scale_1.00006", pose(0.2, (0.3, 0.0, 0.0), scale=1.00006)),
            ("to_3km", pose(0.4, FAR))]


def _poses(N, n1, n2, seed):
    def build():
        rng = np.random.default_rng(seed)
        Ts = [M for _, M in pose_list()]
        pairs = [near_pair(rng, n1, n2, M, centre=(FAR if name == "to_3km" else None)) for name, M in pose_list()]
        return make(pairs, Ts, N)
    return build


case("poses_N300", "scan<1>")(_poses(300, 280, 300, 480))
case("poses_N2049", "sweep<SHARE>", {"window"})(_poses(2049, 700, 900, 481))


def _threshold(N, lens, thres, seed):
    def build():
        rng = np.random.default_rng(seed)
        Ts = [pose(), pose(0.3, (1.5, -0.7, 0.0))] * (len(lens) // 2)
        pairs, marks = [], []
        for (n1, n2), M in zip(lens, Ts):
            a, c = near_pair(rng, n1 - 4, n2 - 4, M)
            a, c, mark = threshold_rows(a, c, M, thres)
            pairs.append((a, c)); marks.append(mark)
        return make(pairs, Ts, N, thres=thres, marks=marks)
    return build


for _t in (0.5, 0.1):      # (n - 1) % 256 >= 192 throughout: the last rows are in the last wave of their block
    case(f"threshold_scan_{_t}", "scan<1>")(_threshold(512, [(250, 510), (510, 255)], _t, 490))
    case(f"threshold_sweep_{_t}", "sweep<SHARE>", {"window"})(_threshold(2049, [(760, 1020), (1020, 760)], _t, 491))
    case(f"threshold_fullscan_{_t}", "sweep<SHARE>", {"full8", "window"})(_threshold(2049, [(250, 2040), (2040, 250)], _t, 492))


def _with_duplicates(c, ranks):
    """the row at rank r + 1 becomes a copy of the row at rank r, for every r (ranks as (row, row + 1) pairs of `ranks`)"""
    for r0, r1 in ranks:
        c[r1] = c[r0]
    return c


@case("duplicates_scan_N1100", "scan<2>")
def _dup_scan():
    """rows 15 / 16 (a chunk seam) and 1023 / 1024 (the tile seam) of pcd2 are the same point, and a moved row of pcd1 lies 1 mm
    from each"""
    rng = np.random.default_rng(500)
    M = pose(0.3, (1.5, -0.7, 0.2))
    a, c = near_pair(rng, 900, 1100, M)
    c = _with_duplicates(c, [(15, 16), (1023, 1024)])
    a[0], a[1] = carried_back(c[[15, 1023]] + F(0.001), M)
    return make([(a, c)], [M], 1100, dup=[(15, 16), (1023, 1024)])


@case("duplicates_sweep_N2049", "sweep<SHARE>", {"window"})
def _dup_sweep():
    """the same at the sorted ranks 15 / 16 and 1023 / 1024 of pcd2"""
    rng = np.random.default_rng(501)
    M = pose(0.3, (1.5, -0.7, 0.2))
    a, c = near_pair(rng, 900, 1500, M)
    o = sr.order(sr.axis_key(sort_code(sc.cloud(a, 2049), sc.cloud(c, 2049)), c))
    dup = [(int(o[15]), int(o[16])), (int(o[1023]), int(o[1024]))]
    c = _with_duplicates(c, dup)
    a[0], a[1] = carried_back(c[[dup[0][0], dup[1][0]]] + F(0.001), M)
    return make([(a, c)], [M], 2049, dup=dup)


def _empty(N):
    def build():
        rng = np.random.default_rng(510 + N)
        lens = [(200, 0), (0, 200), (0, 0), (1, 1), (1, 200), (200, 1), (150, 170)]
        Ts = cycle_poses(len(lens), rng)
        return make([near_pair(rng, a, c, M) for (a, c), M in zip(lens, Ts)], Ts, N)
    return build


case("empty_and_one_point_N300", "scan<1>")(_empty(300))
case("empty_and_one_point_N2049", "sweep<SHARE>", {"empty", "window"})(_empty(2049))


def rotation_poses():
    """-> names, poses: the exact cases of the epilogue's angles"""
    out = [("identity", pose())]
    beyond = pose()
    beyond[2, 0] = F(1.0000001)                      # M[8] > 1: asin(-M[8]) is NaN
    out.append(("m8_above_1", beyond))
    below = pose()
    below[2, 0] = F(-1.5)
    out.append(("m8_below_minus_1", below))
    for name, z in (("half_turn_plus_zero", F(0.0)), ("half_turn_minus_zero", F(-0.0))):
        M = pose()
        M[0, 0] = M[1, 1] = F(-1.0)
        M[1, 0] = z
        out.append((name, M))
    return [n for n, _ in out], [M for _, M in out]


@case("rotations_exact_N16", "scan<1>")
def _rotations_exact():
    rng = np.random.default_rng(520)
    names, Ts = rotation_poses()
    return make([near_pair(rng, 9, 12, pose()) for _ in Ts], Ts, 16, names=names)


def hist_icp_eval_batch(N):
    """The ragged batch of twelve pairs of the icpflow_hist_icp_eval test: dst a shell, src the same shell carried back through a small
    motion the registration can find; both swap states (the src cloud strictly longer: it is the fixed role); at N = 2049 two thin
    boxes turned by 45 degrees, whose fixed cloud hist_icp's sort orders along direction 4.  -> S, D [12, N, 4]"""
    rng = np.random.default_rng(600 + N)
    M = pose(0.02, (0.3, -0.2, 0.0))
    if N == 300:
        lens = [(300, 300), (120, 250), (250, 120), (40, 299), (299, 40), (20, 30), (30, 20), (64, 65), (65, 64), (257, 256), (200, 200), (100, 300)]
        pairs = [near_pair(rng, a, c, M) for a, c in lens]
    else:
        lens = [(2049, 2049), (2049, 600), (600, 2049), (40, 2049), (2049, 40), (300, 1500), (1500, 300), (700, 700), (513, 2049), (30, 25)]
        pairs = [near_pair(rng, a, c, M) for a, c in lens]
        pairs += [(carried_back(sc.thin_box(600, 45.0, seed=1), M), sc.thin_box(1025, 45.0, seed=2)),
                  (carried_back(sc.thin_box(1100, 45.0, seed=3), M), sc.thin_box(700, 45.0, seed=4))]
    return sc.batch(pairs, N)


SWEEP_CASES = [n for n, c in CASES.items() if c["kernel"].startswith("sweep")]
_BUILT, _RESTATED = {}, {}


def get(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]["build"]()
    return _BUILT[name]


def restated(name):
    """-> (per-pair records, dict of the six outputs) of match_eval_restatement.batch, computed once per case"""
    if name not in _RESTATED:
        c = get(name)
        _RESTATED[name] = mr.batch(c["P1"], c["P2"], c["T"], c["thres"])
    return _RESTATED[name]


def runs():
    """(case, no_eval_sweep) of every call the GPU test makes: every case as it comes, every sweep case again as scans"""
    return [(n, False) for n in CASES] + [(n, True) for n in SWEEP_CASES]

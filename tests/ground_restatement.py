"""The reference's ground segmentation restated in plain fp64 numpy: Patchwork++ (patchwork-plusplus/patchworkpp/src/
patchworkpp.cpp and its header) as utils_ground.py:43-66 configures it -- a fresh object per cloud, so the adaptive thresholds
are {0,0,0,0} during the only call; RNR off, R-VPF and TGR on.  The method, quirks included, not Eigen's fp32 bits: the package
needs Eigen and cannot be built here, so this file is what icpflow_ground_segment is held against (COVERAGE.md, named
deviations).  Nothing here imports the product.

segment(points) -> dict(nonground bool [n], table float64 [504, 16] in the layout of include/icpflow_hip.h, patch int [n]
(-1 = not binned), margin [504], gap [504]).  margin: the smallest relative distance of any decision of the patch to its
threshold (every point-plane test of every round, the seed thresholds, 0.707, the signs of mean_z and of heading, the ratio 8,
the product 0.5, the count 1500 and th_dist^2); gap: the smallest (s1 - s2) / s0 of its plane estimates, which makes the normal
well defined.  A decision taken on a NaN plane is IEEE-defined (false) and has no margin.  Also border float64 [n]
(border_distance: the binning's own margin, kept apart from the patches') and rings: per ring that had revert candidates, the
flatness list as it stood (`listed`), the values that ring itself pushed (`own`) and mu; seeds: per patch the seed thresholds
in the order the method forms them (R-VPF's, then R-GPF's); covs: per patch (the covariance behind its last plane, the size of
that set).

Every function takes an optional `params=` (a Params; the defaults are the reference's constants, which the module-level names
keep for the callers that know no other).  The zone layout {2, 4, 4, 4} x {16, 32, 54, 32} is no parameter: the library refuses
any other.  Two hooks state a WRONG rule, so that a CPU test can show that a case notices it: seed_rule= ("z_only": the lowest
DISTINCT heights, a tie counted once; an int: that many seeds in place of num_lpr) and final_plane= ("by", the rule: the last
set is decided by the plane that was fitted before it; "pl": by the plane fitted to it)."""
import dataclasses

import numpy as np

SENSOR_HEIGHT, MIN_RANGE, MAX_RANGE = 1.723, 1.0, 64.0
NUM_ITER, NUM_LPR, NUM_MIN_PTS = 3, 20, 10
TH_SEEDS, TH_DIST, TH_SEEDS_V, TH_DIST_V = 0.125, 0.125, 0.25, 0.1
UPRIGHT, SEED_MARGIN, NEAR_RINGS = 0.707, -1.2, 4
SECTORS, RINGS = (16, 32, 54, 32), (2, 4, 4, 4)
PATCH_BASE, RING_BASE = (0, 32, 160, 376), (0, 2, 6, 10)
PATCHES, COLS = 504, 16
TOO_FEW, NOT_UPRIGHT, FAR, HEADING, ACCEPTED, CANDIDATE = range(6)
TGR_NONE, TGR_REVERTED, TGR_REJECTED = range(3)
MARGIN_BAR, GAP_BAR = 1e-9, 1e-3



@dataclasses.dataclass(frozen=True)
class Params:
    """icpflow_ground_params_t without the layout; the defaults are the constants above"""
    sensor_height: float = SENSOR_HEIGHT
    min_range: float = MIN_RANGE
    max_range: float = MAX_RANGE
    num_iter: int = NUM_ITER
    num_lpr: int = NUM_LPR
    num_min_pts: int = NUM_MIN_PTS
    th_seeds: float = TH_SEEDS
    th_dist: float = TH_DIST
    th_seeds_v: float = TH_SEEDS_V
    th_dist_v: float = TH_DIST_V
    uprightness_thr: float = UPRIGHT
    adaptive_seed_selection_margin: float = SEED_MARGIN

    @property
    def lo(self):
        a, b = self.min_range, self.max_range
        return (a, (7 * a + b) / 8.0, (3 * a + b) / 4.0, (a + b) / 2.0)

    @property
    def ring_size(self):
        lo = self.lo
        return tuple(((lo[k + 1] if k < 3 else self.max_range) - lo[k]) / RINGS[k] for k in range(4))

    @property
    def skip_below(self):
        return self.adaptive_seed_selection_margin * self.sensor_height

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


DEFAULT = Params()

LO = (MIN_RANGE, (7 * MIN_RANGE + MAX_RANGE) / 8.0, (3 * MIN_RANGE + MAX_RANGE) / 4.0, (MIN_RANGE + MAX_RANGE) / 2.0)
RING_SIZE = tuple(((LO[k + 1] if k < 3 else MAX_RANGE) - LO[k]) / RINGS[k] for k in range(4))
SECTOR_SIZE = tuple(2 * np.pi / SECTORS[k] for k in range(4))


def patch_bounds(zone, ring, sector, params=None):
    """(r_lo, r_hi, theta_lo, theta_hi) of a patch"""
    par = params or DEFAULT
    LO, RING_SIZE = par.lo, par.ring_size
    return (LO[zone] + ring * RING_SIZE[zone], LO[zone] + (ring + 1) * RING_SIZE[zone],
            sector * SECTOR_SIZE[zone], (sector + 1) * SECTOR_SIZE[zone])


def patch_index(zone, ring, sector):
    return PATCH_BASE[zone] + ring * SECTORS[zone] + sector


def patch_zone_ring(p):
    zone = 0 if p < 32 else 1 if p < 160 else 2 if p < 376 else 3
    return zone, RING_BASE[zone] + (p - PATCH_BASE[zone]) // SECTORS[zone]


def patch_ids(points, params=None):
    """pc2czm: float32 coordinates, r and theta in double; -1 = the row takes no part"""
    par = params or DEFAULT
    LO, RING_SIZE, MIN_RANGE, MAX_RANGE = par.lo, par.ring_size, par.min_range, par.max_range
    p = np.asarray(points)[:, 0:3].astype(np.float32)
    out = np.full(len(p), -1, dtype=np.int64)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    x, y = p[fin, 0].astype(np.float64), p[fin, 1].astype(np.float64)
    r = np.sqrt(x * x + y * y)
    ok = (r <= MAX_RANGE) & (r > MIN_RANGE)
    fin, x, y, r = fin[ok], x[ok], y[ok], r[ok]
    theta = np.arctan2(y, x)
    theta = np.where(theta > 0, theta, 2 * np.pi + theta)
    zone = np.where(r < LO[1], 0, np.where(r < LO[2], 1, np.where(r < LO[3], 2, 3)))
    lo, rs, ss = np.asarray(LO)[zone], np.asarray(RING_SIZE)[zone], np.asarray(SECTOR_SIZE)[zone]
    ring = np.minimum(((r - lo) / rs).astype(np.int64), np.asarray(RINGS)[zone] - 1)
    sector = np.minimum((theta / ss).astype(np.int64), np.asarray(SECTORS)[zone] - 1)
    out[fin] = np.asarray(PATCH_BASE)[zone] + ring * np.asarray(SECTORS)[zone] + sector
    return out


def border_distance(points, params=None):
    """float64 [n]: how far a row is from the nearest border of the binning, in bins -- |u - round(u)| of its ring coordinate
    u = (r - min_range_k) / ring_size_k (the zone boundaries, min_range and max_range are whole u) and of its sector coordinate
    theta / sector_size_k; for a row out of range its distance to min_range or max_range in rings of the nearest zone.  inf for
    a row with a non-finite coordinate.

    The binning is not part of a patch's margin: a row that changes its bin changes two patches' counts, and the tests hold the
    counts equal on every patch.  Instead tests/test_ground.py asserts, scene by scene, that every row is at least 1e-9 of a
    bin from a border -- seven orders over what a sqrt and an atan2 that is a few ulp off can move it -- except the rows that
    `edges` puts ON a border by construction.  Those are exact in IEEE arithmetic: r is a correctly rounded sqrt of exactly
    representable squares, and atan2 on an axis is the rounded multiple of pi / 2 in every libm."""
    par = params or DEFAULT
    LO, RING_SIZE, MIN_RANGE, MAX_RANGE = par.lo, par.ring_size, par.min_range, par.max_range
    p = np.asarray(points)[:, 0:3].astype(np.float32)
    out = np.full(len(p), np.inf)
    fin = np.flatnonzero(np.isfinite(p).all(axis=1))
    x, y = p[fin, 0].astype(np.float64), p[fin, 1].astype(np.float64)
    r = np.sqrt(x * x + y * y)
    theta = np.arctan2(y, x)
    theta = np.where(theta > 0, theta, 2 * np.pi + theta)
    zone = np.where(r < LO[1], 0, np.where(r < LO[2], 1, np.where(r < LO[3], 2, 3)))
    u = (r - np.asarray(LO)[zone]) / np.asarray(RING_SIZE)[zone]
    v = theta / np.asarray(SECTOR_SIZE)[zone]
    inside = (r <= MAX_RANGE) & (r > MIN_RANGE)
    du = np.where(r > MAX_RANGE, (r - MAX_RANGE) / RING_SIZE[3], np.abs(u - np.round(u)))
    out[fin] = np.where(inside, np.minimum(du, np.abs(v - np.round(v))), du)
    return out


class _Margin:
    def __init__(self):
        self.margin, self.gap, self.seeds = np.inf, np.inf, []

    def rel(self, diff, scale):
        d = np.abs(np.asarray(diff, dtype=np.float64)) / scale
        d = d[~np.isnan(d)]
        if d.size:
            self.margin = min(self.margin, float(d.min()))


NAN_PLANE = dict(mean=np.full(3, np.nan), normal=np.full(3, np.nan), sv=np.full(3, np.nan), d=np.nan)


def estimate_plane(P, plane, mg):
    """an empty set leaves the plane as it was; one point gives 0 / 0: a NaN plane"""
    m = len(P)
    if m == 0:
        return plane
    mean = P.sum(axis=0) / m
    C = P - mean
    with np.errstate(all="ignore"):
        cov = (C.T @ C) / np.float64(m - 1)
    if not np.isfinite(cov).all():
        return dict(mean=mean, normal=np.full(3, np.nan), sv=np.full(3, np.nan), d=np.nan)
    U, S, _ = np.linalg.svd(cov)
    normal = U[:, 2].copy()
    if normal[2] < 0:
        normal = -normal
    mg.gap = min(mg.gap, float((S[1] - S[2]) / S[0]) if S[0] > 0 else 0.0)
    return dict(mean=mean, normal=normal, sv=S, d=-((normal[0] * mean[0] + normal[1] * mean[1]) + normal[2] * mean[2]), cov=cov, size=m)


def seed_threshold(z, zone, th, params=None, seed_rule=None):
    """lpr + th: the double mean of the up to num_lpr (20) lowest z, in zone 0 after the leading z < margin (-1.2) * sensor_height"""
    par = params or DEFAULT
    zs = np.sort(z)
    if zone == 0:
        zs = zs[~(zs < par.skip_below)]
    if seed_rule == "z_only":
        zs = np.unique(zs)
    elif seed_rule is not None:
        par = par.replace(num_lpr=int(seed_rule))
    s, low = 0.0, zs[:par.num_lpr]
    for v in low:
        s += float(v)
    return (s / len(low) if len(low) else 0.0) + th


def plane_dist(plane, P):
    n = plane["normal"]
    with np.errstate(all="ignore"):
        return ((n[0] * P[:, 0] + n[1] * P[:, 1]) + n[2] * P[:, 2]) + plane["d"]


def piecewise_ground(P, zone, mg, params=None, seed_rule=None, final_plane="by"):
    """extract_piecewiseground: -> (ground mask over P, plane, points R-VPF removed, ground count)"""
    par = params or DEFAULT
    NUM_ITER, UPRIGHT = par.num_iter, par.uprightness_thr
    TH_SEEDS, TH_DIST, TH_SEEDS_V, TH_DIST_V = par.th_seeds, par.th_dist, par.th_seeds_v, par.th_dist_v
    assert final_plane in ("by", "pl")
    alive = np.ones(len(P), dtype=bool)
    plane, removed = NAN_PLANE, 0
    for _ in range(NUM_ITER):
        Q = P[alive]
        thr = seed_threshold(Q[:, 2], zone, TH_SEEDS_V, par, seed_rule)
        mg.seeds.append(thr)
        mg.rel(Q[:, 2] - thr, TH_SEEDS_V)
        plane = estimate_plane(Q[Q[:, 2] < thr], plane, mg)
        if zone == 0:
            mg.rel(plane["normal"][2] - UPRIGHT, UPRIGHT)
        if not (zone == 0 and plane["normal"][2] < UPRIGHT):
            break
        d = plane_dist(plane, Q)
        mg.rel(np.abs(d) - TH_DIST_V, TH_DIST_V)
        gone = np.flatnonzero(alive)[np.abs(d) < TH_DIST_V]
        alive[gone] = False
        removed += len(gone)
    Q = P[alive]
    thr = seed_threshold(Q[:, 2], zone, TH_SEEDS, par, seed_rule)
    mg.seeds.append(thr)
    mg.rel(Q[:, 2] - thr, TH_SEEDS)
    plane = estimate_plane(Q[Q[:, 2] < thr], plane, mg)
    g = np.zeros(len(Q), dtype=bool)
    for _ in range(NUM_ITER):
        d = plane_dist(plane, Q)
        mg.rel(d - TH_DIST, TH_DIST)
        g = d < TH_DIST
        plane = estimate_plane(Q[g], plane, mg)
    if final_plane == "pl":                    # the wrong rule: the set of the plane that was fitted last
        g = plane_dist(plane, Q) < TH_DIST
    ground = np.zeros(len(P), dtype=bool)
    ground[np.flatnonzero(alive)[g]] = True
    return ground, plane, removed, int(g.sum())


def segment(points, params=None, seed_rule=None, final_plane="by"):
    par = params or DEFAULT
    NUM_MIN_PTS, UPRIGHT, TH_DIST = par.num_min_pts, par.uprightness_thr, par.th_dist
    pts32 = np.asarray(points)[:, 0:3].astype(np.float32)
    n = len(pts32)
    pid = patch_ids(pts32, par)
    seeds, covs = {}, {}
    nonground = np.ones(n, dtype=bool)
    table = np.zeros((PATCHES, COLS))
    margin, gap = np.full(PATCHES, np.inf), np.full(PATCHES, np.inf)
    order = np.argsort(pid, kind="stable")
    first = np.searchsorted(pid[order], np.arange(PATCHES + 1))
    ground_rows = {}
    listed, p, rings = [], 0, {}
    for zone in range(4):
        for ring in range(RINGS[zone]):
            c = RING_BASE[zone] + ring
            candidates, own = [], []
            for sector in range(SECTORS[zone]):
                p = patch_index(zone, ring, sector)
                rows = order[first[p]:first[p + 1]]
                table[p, 0] = len(rows)
                if len(rows) < NUM_MIN_PTS:
                    continue
                mg = _Margin()
                ground, pl, removed, count = piecewise_ground(pts32[rows].astype(np.float64), zone, mg, par, seed_rule, final_plane)
                seeds[p] = list(mg.seeds)
                if "cov" in pl:
                    covs[p] = (pl["cov"], pl["size"])
                sv, mean, normal = pl["sv"], pl["mean"], pl["normal"]
                upright, not_elevated, flat, near = normal[2] > UPRIGHT, mean[2] < 0.0, sv[2] < 0.0, c < NEAR_RINGS
                heading = 0.0
                for k in range(3):
                    heading += mean[k] * normal[k]
                mg.rel(normal[2] - UPRIGHT, UPRIGHT)
                if upright and near:
                    mg.rel(heading, 1.0)
                    mg.rel(mean[2], 1.0)
                if upright and not_elevated and near:
                    listed.append(float(sv[2]))
                    own.append(float(sv[2]))
                if not upright:
                    code = NOT_UPRIGHT
                elif not near:
                    code = FAR
                elif not heading < 0.0:
                    code = HEADING
                elif not_elevated or flat:
                    code = ACCEPTED
                else:
                    code = CANDIDATE
                    candidates.append(p)
                if code in (FAR, ACCEPTED):
                    nonground[rows[ground]] = False
                ground_rows[p] = rows[ground]
                table[p, 1], table[p, 2:5], table[p, 5:8], table[p, 8:11], table[p, 11] = count, mean, normal, sv, pl["d"]
                table[p, 12], table[p, 13], table[p, 14] = code, TGR_NONE, removed
                margin[p], gap[p] = mg.margin, mg.gap
            if candidates:                     # temporal_ground_revert; the list is cleared only here
                mean_f = stdev_f = np.float64(0.0)
                if len(listed) > 1:            # calc_mean_stdev leaves both 0 for at most one value
                    s = 0.0
                    for v in listed:
                        s += v
                    mean_f = np.float64(s / len(listed))
                    acc = 0.0
                    for v in listed:
                        acc += (v - mean_f) * (v - mean_f)
                    stdev_f = np.sqrt(np.float64(acc / (len(listed) - 1)))
                mu = np.float64(mean_f + 1.5 * stdev_f)
                rings[c] = dict(listed=list(listed), own=own, mu=float(mu))
                for q in candidates:
                    f, s0, s1 = np.float64(table[q, 10]), np.float64(table[q, 8]), np.float64(table[q, 9])
                    with np.errstate(all="ignore"):
                        prob = 1.0 / (1.0 + np.exp((f - mu) / (mu / np.float64(10.0))))
                    m = _Margin()
                    m.rel(table[q, 1] - 1500.5, 1500.0)
                    if table[q, 1] > 1500:
                        m.rel(f - TH_DIST * TH_DIST, TH_DIST * TH_DIST)
                        if f < TH_DIST * TH_DIST:
                            prob = np.float64(1.0)
                    line = s0 / s1 if s1 != 0 else np.finfo(np.float64).max
                    m.rel(line - 8.0, 8.0)
                    prob_line = 0.0 if line > 8.0 else 1.0
                    m.rel(prob_line * prob - 0.5, 0.5)
                    back = bool(prob_line * prob > 0.5)
                    table[q, 13] = TGR_REVERTED if back else TGR_REJECTED
                    if back:
                        nonground[ground_rows[q]] = False
                    margin[q] = min(margin[q], m.margin)
                listed = []
    return dict(nonground=nonground, table=table, patch=pid, margin=margin, gap=gap, border=border_distance(pts32, par), rings=rings, seeds=seeds, covs=covs)


def determined(res, params=None):
    """bool [504]: the patches (of at least num_min_pts points) whose every decision is clear of its threshold"""
    return (res["table"][:, 0] >= (params or DEFAULT).num_min_pts) & (res["margin"] > MARGIN_BAR) & (res["gap"] > GAP_BAR)


def rows_to_compare(res, params=None):
    """bool [n]: the rows whose label is pinned -- every row that is not in an undetermined patch"""
    und = (res["table"][:, 0] >= (params or DEFAULT).num_min_pts) & ~determined(res, params)
    keep = np.ones(len(res["patch"]), dtype=bool)
    inside = res["patch"] >= 0
    keep[inside] = ~und[res["patch"][inside]]
    return keep

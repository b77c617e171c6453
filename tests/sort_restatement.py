"""A plain NumPy restatement of the sorts under every exact search of the library (no GPU, no torch), written from the comments
of csrc/sortclouds.hpp, sortdir.hpp, votekey.hpp, sort.hip and hist.hip (zsort_kernel), not from their code paths:

  * the length of a cloud is its number of rows with w > 0, and only the first n rows are sorted.  Flagged rows are a prefix
    (the pad_segment layout, include/icpflow_hip.h): flags behind an unflagged row are outside the fused path's contract and
    nothing here models them;
  * the moving role is the smaller cloud; the src cloud moves unless it is STRICTLY longer (utils_match.py:139-146);
  * the axis key code of a pair comes from the fixed role's first ny rows (`choose_code`), the key of a point from `axis_key`,
    the vote's key from `vote_key_record` / `vote_key`;
  * the order is stable ascending by (key + 0.0f, row): `order`.

Every float32 operation is a NumPy float32 operation on float32 operands, so each is rounded by itself, as the library's are under
-ffp-contract=off.  The one fused operation, fmaf, is `fma32`: the product of two float32 numbers is exact in float64, the sum with
the addend is formed by an error-free two-sum, the float64 result is rounded TO ODD with the error's help, and one rounding to
float32 follows -- float64 carries 29 bits more than float32, more than the two that rounding to odd needs, so that last rounding is
the correct rounding of the exact a * b + c.  tests/test_sort_restatement.py checks it against exact rationals.
"""
import numpy as np

F = np.float32
INF = F(np.inf)

SORT_DIR_MIN_N = 1025          # fixed clouds of at least this many rows choose among the direction keys ...
SORT_DIR_MIN_MOVING = 512      # ... against a moving cloud of at least this many
SORT_DIR_BINS = 512
SORT_DIR_BIN = F(0.1)
SORT_CODES = 9
WIDE_MIN_EXTENT = F(8.0)
WIDE_MIN_POINTS = 4096
SLAB_STRIDE = F(1024.0)
# sort_dir: cos / sin 22.5 deg and cos 45 deg as the float32 literals of csrc/sortdir.hpp (rounded towards zero)
_C1, _S1, _C2 = F(0.9238795), F(0.3826834), F(0.7071067)
SORT_DIRS = {3: (_C1, _S1), 4: (_C2, _C2), 5: (_S1, _C1), 6: (-_S1, _C1), 7: (-_C2, _C2), 8: (-_C1, _S1)}


def f32(x):
    return np.asarray(x, dtype=F)


def fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the correctly rounded float32 of the exact a * b + c (finite operands)."""
    a, b, c = np.broadcast_arrays(f32(a), f32(b), f32(c))
    p = a.astype(np.float64) * b.astype(np.float64)          # exact: 24 + 24 bits, exponents far inside float64's
    cc = c.astype(np.float64)
    s = p + cc
    bb = s - p
    err = (p - (s - bb)) + (cc - bb)                         # two-sum: s + err = p + cc exactly
    odd = (s.view(np.int64) & 1) != 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & ~odd, np.nextafter(s, toward), s)   # round to odd
    return s.astype(F)


def canonical(keys):
    """key + 0.0f: -0.0 becomes +0.0, everything else stays."""
    return f32(keys) + F(0.0)


def order(keys):
    """rows in stable ascending order by (canonical key, row)"""
    return np.argsort(canonical(keys), kind="stable")


def length(cloud):
    """rows with w > 0 of one cloud [N, 4]"""
    return int((f32(cloud)[:, 3] > 0).sum())


def roles(src, dst):
    """-> (nA, nC, swap, moving cloud, nx, fixed cloud, ny) of one pair; swap: the src cloud is strictly longer and is the fixed one"""
    nA, nC = length(src), length(dst)
    swap = nA > nC
    return (nA, nC, int(swap)) + ((dst, nC, src, nA) if swap else (src, nA, dst, nC))


def box_of(rows):
    """(min x y z, max x y z) float32 of rows [n, >= 3]; an empty set gives (+inf, -inf)"""
    rows = f32(rows)[:, :3]
    if len(rows) == 0:
        return np.array([INF] * 3 + [-INF] * 3, F)
    return np.concatenate([rows.min(axis=0), rows.max(axis=0)]).astype(F)


def legacy_code(box):
    with np.errstate(invalid="ignore"):
        e = box[3:6] - box[0:3]
        return 0 if (e[0] >= e[1] and e[0] >= e[2]) else (1 if e[1] >= e[2] else 2)


def axis_key(code, xyz):
    """the sort key of points [n, 3] under `code`: a coordinate (0 .. 2) or fmaf(uy, y, fl(ux * x)) (3 .. 8)"""
    xyz = f32(xyz)
    if code < 3:
        return xyz[:, code].copy()
    ux, uy = SORT_DIRS[code]
    return fma32(uy, xyz[:, 1], ux * xyz[:, 0])


def dir_scores(rows, box):
    """choose_sort_code's nine scores: the sum of c * c over the 0.1 m key bins holding c > 1 of the rows"""
    rows = f32(rows)[:, :3]
    half = F(0.5)
    centre = half * (box[0:3] + box[3:6])
    e = box[3:6] - box[0:3]
    R = half * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], dtype=F) + F(0.05)
    inv = F(1.0) / np.maximum(SORT_DIR_BIN, F(2.0) * R / F(SORT_DIR_BINS))
    d = rows - centre                                         # (q.x - cx, q.y - cy, q.z - cz), float32
    scores = []
    for code in range(SORT_CODES):
        k = axis_key(code, d)
        bins = np.clip(np.trunc((k + R) * inv).astype(np.int64), 0, SORT_DIR_BINS - 1)
        c = np.bincount(bins, minlength=SORT_DIR_BINS).astype(np.int64)
        scores.append(int((c[c > 1] ** 2).sum()))
    return scores


def choose_code(fixed_rows, nx, dir_keys=True):
    """The key code of a pair from the fixed role's first ny rows [ny, >= 3] and the moving role's length.
    -> (code, info); info: legacy, scores (None where no direction may be chosen), and the two distances of the decision from
    flipping: margin = 9 s_legacy - 10 s_best (>= 0 iff another key may replace the longest axis; s_best the smallest score of the
    OTHER codes) and gap = the second smallest score minus the smallest."""
    fixed_rows = f32(fixed_rows)
    ny = len(fixed_rows)
    box = box_of(fixed_rows)
    legacy = legacy_code(box)
    info = dict(legacy=legacy, scores=None, margin=None, gap=None, box=box)
    if not (dir_keys and ny >= SORT_DIR_MIN_N and nx >= SORT_DIR_MIN_MOVING):
        return legacy, info
    s = dir_scores(fixed_rows, box)
    best, sb = legacy, s[legacy]
    for c in range(SORT_CODES):                               # the first strict minimum, starting from the legacy code
        if s[c] < sb:
            best, sb = c, s[c]
    code = best if (best != legacy and 10 * sb <= 9 * s[legacy]) else legacy
    others = sorted(s[c] for c in range(SORT_CODES) if c != legacy)
    ranked = sorted(s)
    info.update(scores=s, margin=9 * s[legacy] - 10 * others[0], gap=ranked[1] - ranked[0])
    return code, info


def axis_sorted_pair(src, dst, dir_keys=True, swap_allowed=True):
    """What the axis sort leaves of one pair of clouds [N, 4] (no pre-pose) -> dict(nA, nC, swap, code, info,
    fixed_ids, moving_ids, fixed_rows, moving_rows): ids = the rows of a role's cloud in sorted order, rows = (x, y, z) in that order.
    swap_allowed = False: the entry points that take the src cloud as the moving one whatever the lengths."""
    src, dst = f32(src), f32(dst)
    nA, nC, swap, moving, nx, fixed, ny = roles(src, dst)
    if not swap_allowed and swap:
        swap, moving, nx, fixed, ny = 0, src, nA, dst, nC
    code, info = choose_code(fixed[:ny, :3], nx, dir_keys)
    fid = order(axis_key(code, fixed[:ny, :3]))
    mid = order(axis_key(code, moving[:nx, :3]))
    return dict(nA=nA, nC=nC, swap=swap, code=code, info=info, fixed_ids=fid, moving_ids=mid, fixed_rows=fixed[fid, :3],
                moving_rows=moving[mid, :3], nx=nx, ny=ny)


def vote_key_record(src, dst, h_box):
    """The vote's key parameters of one pair (wide, uaxis, u0, z0, h) from the flagged rows of both clouds and the z range of the
    vote box (the last z edge minus the first, float32)."""
    src, dst = f32(src), f32(dst)
    nA, nC = length(src), length(dst)
    h = np.maximum(F(h_box), F(1e-3))
    if nA + nC <= WIDE_MIN_POINTS:
        return (0, 0, F(0), F(0), h)
    box = box_of(np.concatenate([src[:nA][src[:nA, 3] > 0], dst[:nC][dst[:nC, 3] > 0]]))
    lo, hi = box[0:3], box[3:6]
    ua = 0 if (hi[0] - lo[0]) >= (hi[1] - lo[1]) else 1
    eu, ez = hi[ua] - lo[ua], hi[2] - lo[2]
    wide = bool(eu > WIDE_MIN_EXTENT and eu < F(1000.0) and ez < F(250.0) * h)
    return (int(wide), ua, lo[ua], lo[2], h)


def vote_slab(rec, xyz):
    """(z - z0) / h in float32, before the floor: the number whose integer values are the slab borders"""
    _, _, _, z0, h = rec
    return (f32(xyz)[:, 2] - z0) / h


def vote_key(rec, xyz):
    xyz = f32(xyz)
    wide, ua, u0, _, _ = rec
    if not wide:
        return xyz[:, 2].copy()
    s = np.floor(vote_slab(rec, xyz))
    u = np.minimum(np.maximum(xyz[:, ua] - u0, F(0.0)), SLAB_STRIDE - F(1.0))
    return fma32(s, SLAB_STRIDE, u)


def z_sorted_cloud(cloud, rec):
    """What the vote's sort leaves of one cloud [N, 4] -> (n, rows [n, 4]): the flagged rows in key order, the key in w."""
    cloud = f32(cloud)
    n = length(cloud)
    key = vote_key(rec, cloud[:n, :3])
    ids = order(key)
    out = cloud[:n][ids].copy()
    out[:, 3] = canonical(key)[ids]
    return n, out

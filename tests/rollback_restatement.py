"""A plain NumPy restatement of the roll-back (rows a-8 / a-9: the tail of icpflow_apply_icp and icpflow_hist_icp; no GPU, no torch),
written from utils_icp.py:20-48, utils_match.py:152-154 and the comments of csrc/pose.hip (compose_kernel, select_kernel),
posefuse.hpp (final_pose) and nn.hip (MODE_CHECK, SWEEP_CHECK), not from the kernels' paths.  Given the floats (R, T) that the ICP
leaves -- icpflow_icp exports them --, everything behind them is a closed statement:

  * compose: M = [[R^T, T], [0 0 0 1]] * init in float32, per entry one product and three fmaf, k ascending (`compose`);
  * the check moves every valid row of the MOVING cloud by a pose (match_eval_restatement.moved: the same affine form as
    MODE_EVAL's, common.hpp affine_apply) and takes the smallest float32 squared distance to the valid rows of the fixed cloud
    (match_eval_restatement.min_d2: common.hpp sqdist), the distance is its float32 square root (`row_distances`);
  * a mean is float32(S) / float32(n): S the library's float64 sum of those distances in an order of its own, n the valid count
    of the MOVING cloud (`mean_interval`: every value the summation order allows);
  * the rule: the initial pose where e1 >= e0, else M; a NaN on either side keeps M (`decide`);
  * hist_icp returns, for the pairs it swapped, the affine inverse of the selected pose: evaluated in float64, rounded to float32,
    bottom row 0 0 0 1 (`exact_inverse`, `inverse_bound`: the exact inverse in rationals and how far from it the call may be).

`expected` puts it together.  The paths a call takes -- which of the three finishes, scan or sweep, queries per lane -- are restated
at the end from csrc/api.hip (search_scratch, run_icp_and_select) and icp.hip (launch_icp: `speculative`)."""
import math
from fractions import Fraction

import numpy as np

import match_eval_cases as mc
import match_eval_restatement as mr

F = np.float32
fma32 = mr.fma32
length = mr.length
share_instantiation, direction_path, scan_queries_per_lane = mc.share_instantiation, mc.direction_path, mc.scan_queries_per_lane
HIST_ITERS, MAX_SORT_N, SWEEP_MIN_N = 128, mc.MAX_SORT_N, 64      # kernels.hpp kHistIters; api.hip kMaxSortN, search_scratch
U64 = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ compose
def compose(R, T, init):
    """R [3, 3] (row-vector convention y = x R + T), T [3], init [4, 4] float32 -> [[R^T, T], [0 0 0 1]] * init, float32 [4, 4]:
    acc = A[i, 0] * I[0, j]; acc = fmaf(A[i, k], I[k, j], acc) for k = 1, 2, 3"""
    A = np.zeros((4, 4), F)
    A[:3, :3] = np.asarray(R, F).reshape(3, 3).T
    A[:3, 3] = np.asarray(T, F).reshape(3)
    A[3, 3] = 1
    I = np.asarray(init, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        acc = A[:, 0:1] * I[0:1, :]
        for k in (1, 2, 3):
            acc = fma32(A[:, k:k + 1], I[k:k + 1, :], acc)
    return acc.astype(F)


# ------------------------------------------------------------------------------------------------ the two means
def row_distances(moving, fixed, pose):
    """the float32 distance of every valid row of `moving` [N, 4], moved by `pose`, to its nearest valid row of `fixed` [N, 4]"""
    moving, fixed = np.asarray(moving, F), np.asarray(fixed, F)
    n, m = length(moving), length(fixed)
    with np.errstate(all="ignore"):
        return np.sqrt(mr.min_d2(mr.moved(moving[:n, :3], pose), fixed[:m, :3]))


def mean_interval(d, empty_target=False):
    """-> (low, high) float32: what float32(S) / float32(n) can be when S is the float64 sum of the n distances d in ANY order
    (match_eval_restatement.sum_bounds with A = S*: the terms are non-negative).  No row: 0 / 0 = NaN.  Without a target the scans
    sum +inf and the sweeps 0 (the search finds nothing and adds nothing): both are given, (0 / n, +inf / n)."""
    n = len(d)
    with np.errstate(all="ignore"):
        if empty_target and n > 0:
            return F(0) / F(n), F(np.inf) / F(n)
    d = np.asarray(d, np.float64)
    S = math.fsum(d)
    nz = d[(d != 0) & np.isfinite(d)]
    if len(nz) == len(d[d != 0]) and len(nz):
        # Every partial sum of any subset is a multiple of the smallest term's float32 step 2^(emin - 24) and below n 2^emax
        # (frexp's exponents): where that is within 53 bits, no addition rounds in any order and the float64 sum IS S*.  (A sum of
        # a few float32 numbers often lies exactly half way between two float32 numbers: the general bound would then straddle
        # a rounding boundary that the library, which rounds S* itself to nearest even, never meets.)
        e = np.frexp(nz)[1]
        if int(e.max()) - int(e.min()) + 24 + math.ceil(math.log2(max(n, 2))) <= 53:
            with np.errstate(all="ignore"):
                v = F(S) / F(n)
            return v, v
    return mr.sum_bounds(S, S, n)


def determined(iv):
    lo, hi = iv
    return bool(F(lo).view(np.uint32) == F(hi).view(np.uint32)) or bool(np.isnan(lo) and np.isnan(hi))


def rule(e0, e1):
    """utils_icp.py:34 on float32 numbers: the initial pose where e1 >= e0; a NaN on either side keeps the ICP's"""
    with np.errstate(all="ignore"):
        return bool(F(e1) >= F(e0))


def decide(iv0, iv1):
    """-> dict(rolled: True / False / None, decided, tie, certain).  decided: both means are one float32 number each.  certain: the
    rule gives the same answer at every combination of the ends (a decided pair is certain; an undecided one may be)."""
    dec = determined(iv0) and determined(iv1)
    answers = {rule(a, b) for a in iv0 for b in iv1}
    certain = len(answers) == 1
    with np.errstate(all="ignore"):
        tie = dec and bool(F(iv0[0]) == F(iv1[0]))
    return dict(rolled=answers.pop() if certain else None, decided=dec, tie=tie, certain=certain)


# ------------------------------------------------------------------------------------------------ the inverse of swapped pairs
def _frac(M):
    return [[Fraction(float(x)) for x in row] for row in np.asarray(M, F).reshape(4, 4)]


def exact_inverse(P):
    """The affine inverse of the sixteen float32 entries of P, in rationals -> (inverse: 4 x 4 list of Fraction with the bottom
    row 0 0 0 1, kappa: the 1-norm condition number of the 3 x 3 block, a Fraction).  The bottom row of P is not read (the kernel
    does not read it either).  A singular block: ZeroDivisionError."""
    m = _frac(P)
    a, b, c, d, e, f, g, h, i = m[0][0], m[0][1], m[0][2], m[1][0], m[1][1], m[1][2], m[2][0], m[2][1], m[2][2]
    cof = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = a * cof[0][0] + b * cof[1][0] + c * cof[2][0]
    inv3 = [[x / det for x in row] for row in cof]
    t = [m[0][3], m[1][3], m[2][3]]
    out = [inv3[r] + [-sum(inv3[r][k] * t[k] for k in range(3))] for r in range(3)] + [[Fraction(0)] * 3 + [Fraction(1)]]
    norm1 = lambda q: max(sum(abs(q[r][k]) for r in range(3)) for k in range(3))     # noqa: E731
    return out, norm1([row[:3] for row in m[:3]]) * norm1(inv3)


def ulp32(x):
    """the spacing of float32 in the binade of |x| (x a Fraction or a float); 2^-149 at and below the subnormals"""
    x = abs(float(x))
    if x == 0.0 or not math.isfinite(x):
        return Fraction(2) ** -149
    return Fraction(2) ** max(math.frexp(x)[1] - 1 - 23, -149)


def inverse_bound(P):
    """-> (exact inverse, bound): |call - exact| <= bound entry by entry.  One rounding to float32, ulp32(exact) / 2, plus what the
    float64 evaluation (cofactors, determinant, reciprocal, products: a handful of roundings each, contracted or not) can be
    off by: 8 * 2^-53 * |I_ij| * kappa in the 3 x 3 block, 8 * 2^-53 * sum_j |I_ij| |t_j| in the translation; the bottom row
    is written, not computed: 0."""
    inv, kappa = exact_inverse(P)
    t = [abs(Fraction(float(x))) for x in np.asarray(P, F).reshape(4, 4)[:3, 3]]
    u8 = Fraction(8) * Fraction(2) ** -53
    bound = [[ulp32(inv[r][k]) / 2 + u8 * abs(inv[r][k]) * kappa for k in range(3)] +
             [ulp32(inv[r][3]) / 2 + u8 * sum(abs(inv[r][k]) * t[k] for k in range(3))] for r in range(3)] + [[Fraction(0)] * 4]
    return inv, bound


def round32(x):
    """the float32 nearest to the Fraction x (of two equally near ones either)"""
    c = F(float(x))
    cands = [np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))]
    return min(cands, key=lambda v: abs(Fraction(float(v)) - x) if np.isfinite(v) else Fraction(10) ** 60)


def check_inverse(got, P):
    """-> (ok, the largest |got - exact| / bound over the twelve computed entries, entries that are not the correctly rounded exact
    value); the bottom row must be 0 0 0 1 exactly"""
    inv, bound = inverse_bound(P)
    got = np.asarray(got, F).reshape(4, 4)
    ok, worst, misrounded = same_bits(got[3], np.array([0, 0, 0, 1], F)), 0.0, 0
    for r in range(3):
        for k in range(4):
            err = abs(Fraction(float(got[r, k])) - inv[r][k])
            ok = ok and err <= bound[r][k]
            worst = max(worst, float(err / bound[r][k]))
            misrounded += int(F(got[r, k]).view(np.uint32) != F(round32(inv[r][k])).view(np.uint32) and not (got[r, k] == 0 and inv[r][k] == 0))
    return ok, worst, misrounded


# ------------------------------------------------------------------------------------------------ the whole tail
def init_distances(moving, fixed, init):
    """per pair: the rows' distances under the initial pose (they do not depend on the ICP: computed once per batch)"""
    return [row_distances(a, c, P) for a, c, P in zip(moving, fixed, init)]


def expected(moving, fixed, init, R, T, swapped=None, d0=None):
    """The batch by ROLE (moving, fixed: [B, N, 4]; a pair that hist_icp swaps has its clouds exchanged by the caller), the initial
    poses [B, 4, 4] and the ICP's (R [B, 3, 3], T [B, 3]) -> list of dicts per pair: M (the composed pose), e0 / e1 (intervals),
    rolled / decided / tie / certain (`decide`), selected (init or M by the rule; None where the rule is not certain), n.
    swapped [B] bool: for those pairs the caller compares with `check_inverse(got, selected)`."""
    out = []
    d0 = init_distances(moving, fixed, init) if d0 is None else d0
    for b in range(len(moving)):
        M = compose(R[b], T[b], init[b])
        empty = length(fixed[b]) == 0
        iv0 = mean_interval(d0[b], empty)
        bad = not np.isfinite(M[:3]).all()
        with np.errstate(all="ignore"):
            d1 = np.full(len(d0[b]), np.nan, F) if bad else row_distances(moving[b], fixed[b], M)
            iv1 = mean_interval(d1, empty)
        r = decide(iv0, iv1)
        r.update(S0=math.fsum(np.asarray(d0[b], np.float64)), S1=math.fsum(np.asarray(d1, np.float64)), other=length(fixed[b]))
        if empty and len(d0[b]):          # 0 >= 0 and +inf >= +inf: the initial pose on every path, whatever the sums are called
            r = dict(rolled=True, decided=True, tie=True, certain=True)
        r.update(M=M, e0=iv0, e1=iv1, n=len(d0[b]), swapped=bool(swapped[b]) if swapped is not None else False,
                 selected=None if r["rolled"] is None else (np.asarray(init[b], F) if r["rolled"] else M))
        out.append(r)
    return out


def rule_with_the_other_length(r):
    """what the rule would say of a record of `expected` if the pair's sums were divided by the FIXED cloud's length -- the wrong one
    for a pair that hist_icp swapped.  (Only the rounding of the two quotients can tell the lengths apart.)"""
    with np.errstate(all="ignore"):
        return rule(F(r["S0"]) / F(r["other"]), F(r["S1"]) / F(r["other"]))


# ------------------------------------------------------------------------------------------------ the paths
def search_mode(N, search="auto", arith="fp64"):
    """api.hip search_scratch -> 'scan' | 'grid' | 'sweep'"""
    mode = "scan" if arith == "fp32_reference" else search
    if mode == "auto":
        mode = "sweep" if SWEEP_MIN_N <= N <= MAX_SORT_N else "scan"
    if mode == "sweep" and N > MAX_SORT_N:
        mode = "scan"
    return mode


def sweep_check(N, search="auto", flags=(), arith="fp64"):
    """run_icp_and_select: the check runs as sweeps over the ICP's sorted clouds (and the finish is fused)"""
    return search_mode(N, search, arith) == "sweep" and "no_check_sweep" not in flags


def finish(N, search="auto", flags=(), arith="fp64", max_iterations=50, stop_mode=0):
    """-> 'history' (F1) | 'state' (F2) | 'unfused' (F3)"""
    if not sweep_check(N, search, flags, arith):
        return "unfused"
    speculative = stop_mode == 0 and "no_speculative" not in flags and 2 <= max_iterations <= HIST_ITERS
    return "history" if speculative and arith == "fp64" else "state"


def check_path(B, N, lens, search="auto", flags=(), arith="fp64", max_iterations=50, stop_mode=0):
    """-> dict(finish, kernel: 'scan<Q>' | 'sweep<plain>' | 'sweep<SHARE>', dirs: per pair direction_path(moving, fixed) on sweeps)"""
    fin = finish(N, search, flags, arith, max_iterations, stop_mode)
    if fin == "unfused":
        return dict(finish=fin, kernel=f"scan<{scan_queries_per_lane(N, B)}>", dirs=None)
    return dict(finish=fin, kernel="sweep<SHARE>" if share_instantiation(B, N) else "sweep<plain>",
                dirs=[direction_path(nq, nt, B, N) for nq, nt in lens])

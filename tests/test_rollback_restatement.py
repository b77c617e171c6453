"""tests/rollback_restatement.py against the oracle, and every claim of tests/rollback_cases.py in numbers (no GPU).

The oracle (oracle.reference_path.apply_icp, Kabsch in float64 as the library's) supplies an ICP pose for every case; with it
  * the restated means agree with the oracle's float32-summed ones within 2 (n - 1) 2^-24 e: the oracle adds n float32 terms one
    after the other, each addition rounds by at most 2^-24 of a partial sum <= S, and the restatement's own sum is exact;
  * the restated decision is the oracle's wherever the oracle's two means are farther apart than those bounds together;
  * every pair of every case is DECIDED: both means are one float32 number whatever order the library sums in.

`compose` is compose_kernel's fmaf chain; the oracle's tiny_mm rounds every product and every sum.  The two are the same float32
numbers where no intermediate value needs rounding (poses on a binary lattice: quarter turns, dyadic translations) and where the
products are by 0 and 1 (the 3 x 3 block under the production's identity + translation): there the comparison is bit for bit, and
it pins every index and the transposition.  Elsewhere the two differ by the roundings the fused form saves, at most three per entry:
|difference| <= 3 * 2^-24 * sum_k |A_ik| |I_kj|."""
import numpy as np
import pytest
import torch

import match_eval_restatement as mr
import rollback_cases as rc
import rollback_restatement as rr
from oracle import reference_path as rp

F = np.float32
_ORACLE = {}


def oracle(name):
    """-> dict(R, T, M (composed by the oracle, before the roll-back), e0, e1, rolled, iterations, init) for a case; the second
    application: the oracle's own first result is the initial pose"""
    if name in _ORACLE:
        return _ORACLE[name]
    c = rc.get(name)
    a = rp.default_args(max_points=c["S"].shape[1], thres_dist=rc.THRES)
    S, D, init = torch.from_numpy(c["S"]), torch.from_numpy(c["D"]), torch.from_numpy(c["init"])
    if c.get("second"):
        init = rp.apply_icp(a, S, D, init, max_iterations=c["max_iterations"], kabsch_dtype=torch.float64)
    moved = rp.transform_points_batch(S, init)
    with np.errstate(all="ignore"):
        sol = rp.iterative_closest_point(moved, D, thres=rc.THRES, max_iterations=c["max_iterations"], relative_rmse_thr=c["rel"],
                                         kabsch_dtype=torch.float64)
        A = torch.zeros(len(S), 4, 4)
        A[:, :3, :3], A[:, :3, 3], A[:, 3, 3] = sol.R.transpose(1, 2), sol.T, 1.0
        M = rp.tiny_mm(A, init)
        valid = S[:, :, 3] > 0
        e0 = (rp.nearest_neighbor_batch(moved, D)[1] * valid).sum(1) / valid.sum(1)
        e1 = (rp.nearest_neighbor_batch(rp.transform_points_batch(S, M), D)[1] * valid).sum(1) / valid.sum(1)
    _ORACLE[name] = dict(R=sol.R.numpy(), T=sol.T.numpy(), M=M.numpy(), e0=e0.numpy(), e1=e1.numpy(), rolled=(e1 >= e0).numpy(),
                         iterations=sol.iterations, init=init.numpy())
    return _ORACLE[name]


_EXPECTED = {}


def expected(name):
    if name not in _EXPECTED:
        c, o = rc.get(name), oracle(name)
        _EXPECTED[name] = rr.expected(c["S"], c["D"], o["init"], o["R"], o["T"])
    return _EXPECTED[name]


SMALL = ["decoy_N1024", "poses_N1024", "width_N63", "width_N64", "width_N512", "width_N513", "batch_B65_N64", "stop_65_N64",
         "second_decoy_N1024", "second_ragged_N512"]


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", SMALL)
def test_means_and_decision_against_the_oracle(name):
    c, o = rc.get(name), oracle(name)
    checked = 0
    for b, (n, m) in enumerate(rc.lens_of(c)):
        iv0 = rr.mean_interval(rr.row_distances(c["S"][b], c["D"][b], o["init"][b]))
        iv1 = rr.mean_interval(rr.row_distances(c["S"][b], c["D"][b], o["M"][b]))
        tol0, tol1 = (2 * (n - 1) * 2.0 ** -24 * float(e) for e in (o["e0"][b], o["e1"][b]))
        assert abs(float(iv0[0]) - float(o["e0"][b])) <= tol0 and abs(float(iv0[1]) - float(o["e0"][b])) <= tol0, (name, b, iv0, o["e0"][b])
        assert abs(float(iv1[0]) - float(o["e1"][b])) <= tol1 and abs(float(iv1[1]) - float(o["e1"][b])) <= tol1, (name, b, iv1, o["e1"][b])
        if abs(float(o["e1"][b]) - float(o["e0"][b])) > tol0 + tol1:
            r = rr.decide(iv0, iv1)
            assert r["certain"] and r["rolled"] == bool(o["rolled"][b]), (name, b, r, o["e0"][b], o["e1"][b])
            checked += 1
    # (the second application is made of pairs whose means differ by less than the oracle's own summation error: nothing to ask there)
    assert checked >= (0 if c.get("second") else len(c["S"]) // 2), (name, checked)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_every_pair_is_decided_under_the_oracles_poses(name):
    """the share of decided pairs is 100 % for the chosen seeds: no float32 rounding boundary inside an interval"""
    ex = expected(name)
    undecided = [b for b, r in enumerate(ex) if not r["decided"]]
    assert not undecided, (name, undecided, [(ex[b]["e0"], ex[b]["e1"]) for b in undecided])


# ------------------------------------------------------------------------------------------------ compose
def lattice_poses(rng, count):
    """quarter turns about the three axes and translations on the lattice of 1/64: every product and partial sum is exact"""
    turns = []
    for axis in range(3):
        for q in range(4):
            c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][q]
            R = np.eye(3)
            i, j = [(1, 2), (0, 2), (0, 1)][axis]
            R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
            turns.append(R)
    out = []
    for _ in range(count):
        P = np.eye(4)
        P[:3, :3] = turns[rng.integers(12)] @ turns[rng.integers(12)]
        P[:3, 3] = rng.integers(-4096, 4097, 3) / 64.0
        out.append(P.astype(F))
    return out


def as_RT(P):
    """the (R, T) of the row-vector convention whose [[R^T, T], [0 0 0 1]] is P"""
    return np.ascontiguousarray(P[:3, :3].T), np.ascontiguousarray(P[:3, 3])


def tiny(A, I):
    return rp.tiny_mm(torch.from_numpy(np.asarray(A, F))[None], torch.from_numpy(np.asarray(I, F))[None])[0].numpy()


def test_compose_equals_tiny_mm_bit_for_bit_where_nothing_is_rounded():
    rng = np.random.default_rng(11)
    ps = lattice_poses(rng, 64)
    seen = set()
    for A, I in zip(ps[:32], ps[32:]):
        got = rr.compose(*as_RT(A), I)
        assert rr.same_bits(got, tiny(A, I)), (A, I, got)
        seen.add(got.tobytes())
        assert not rr.same_bits(got, tiny(I, A)) or rr.same_bits(A, I) or np.array_equal(tiny(A, I), tiny(I, A))
    assert len(seen) >= 30
    # a transposed index in either factor would show: the product is not the product of a transpose
    A, I = ps[1], ps[40]
    assert not rr.same_bits(rr.compose(*as_RT(A), I), tiny(A, I.T.copy())) and not rr.same_bits(rr.compose(*as_RT(A), I), tiny(A.T.copy(), I))


def test_compose_against_tiny_mm_on_general_poses():
    """the 3 x 3 block and the bottom row under identity + translation bit for bit; every entry within the three saved roundings"""
    rng = np.random.default_rng(12)
    differing = total = 0
    for k in range(200):
        yaw, tilt = rng.uniform(-np.pi, np.pi), rng.normal(0, 1e-3, 2)
        A = rc.pose(yaw, rng.uniform(-3, 3, 3)).astype(np.float64)
        A[2, 0], A[2, 1] = tilt
        A[0, 2], A[1, 2] = -tilt
        A = A.astype(F)
        I = rc.pose(0.0, rng.uniform(-3, 3, 3)) if k % 2 == 0 else rc.pose(rng.uniform(-np.pi, np.pi), rng.uniform(-3000, 3000, 3))
        got, ref = rr.compose(*as_RT(A), I), tiny(A, I)
        bound = 3 * 2.0 ** -24 * (np.abs(A.astype(np.float64)) @ np.abs(I.astype(np.float64)))
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= bound).all(), (k, got, ref)
        if k % 2 == 0:
            assert rr.same_bits(got[:, :3], ref[:, :3]) and rr.same_bits(got[3], ref[3]), (k, got, ref)
        differing += int((rr.bits(got) != rr.bits(ref)).sum())
        total += 16
    print(f"compose vs tiny_mm on general poses: {differing} of {total} entries differ in the last bits")


def test_compose_is_the_fmaf_chain_entry_by_entry():
    """against a scalar evaluation with Python's exact rationals: product, then three fused steps, each rounded once"""
    from fractions import Fraction
    rng = np.random.default_rng(13)
    r32 = lambda x: rr.round32(x)                                  # noqa: E731
    for _ in range(6):
        A = rc.pose(rng.uniform(-3, 3), rng.uniform(-50, 50, 3))
        I = rc.pose(rng.uniform(-3, 3), rng.uniform(-3000, 3000, 3))
        got = rr.compose(*as_RT(A), I)
        for i in range(4):
            for j in range(4):
                acc = r32(Fraction(float(A[i, 0])) * Fraction(float(I[0, j])))
                for k in (1, 2, 3):
                    acc = r32(Fraction(float(A[i, k])) * Fraction(float(I[k, j])) + Fraction(float(acc)))
                assert F(acc).view(np.uint32) == got[i, j].view(np.uint32), (i, j, acc, got[i, j])


# ------------------------------------------------------------------------------------------------ the inverse
def test_exact_inverse_against_numpy():
    rng = np.random.default_rng(14)
    poses = [P for _, P, _ in rc.init_poses()] + [rc.pose(rng.uniform(-3, 3), rng.uniform(-100, 100, 3), scale=s) for s in (1.0, 0.7, 1.3)]
    for P in poses:
        inv, kappa = rr.exact_inverse(P)
        mine = np.array([[float(x) for x in row] for row in inv])
        assert np.allclose(mine, np.linalg.inv(P.astype(np.float64)), rtol=1e-12, atol=1e-12), P
        assert 1.0 <= float(kappa) < 10.0
        # the float64 evaluation of the kernel's formulas, rounded to float32, is inside the bound (and so is the exact value)
        got = np.linalg.inv(P.astype(np.float64)).astype(F)
        got[3] = [0, 0, 0, 1]
        ok, worst, _ = rr.check_inverse(got, P)
        assert ok and worst <= 1.0, (P, worst)
        wrong = got.copy()
        wrong[0, 3] = np.nextafter(np.nextafter(wrong[0, 3], F(np.inf)), F(np.inf))
        assert not rr.check_inverse(wrong, P)[0]
        assert not rr.check_inverse(got.T.copy(), P)[0] or np.array_equal(got, got.T)


def test_decide():
    one = lambda x: (F(x), F(x))                                     # noqa: E731
    assert rr.decide(one(1.0), one(1.0)) == dict(rolled=True, decided=True, tie=True, certain=True)
    assert rr.decide(one(1.0), one(np.nextafter(F(1.0), F(0)))) == dict(rolled=False, decided=True, tie=False, certain=True)
    assert rr.decide(one(np.nan), one(1.0))["rolled"] is False and rr.decide(one(1.0), one(np.nan))["rolled"] is False
    assert rr.decide(one(np.inf), one(np.inf))["rolled"] is True
    wide = (F(1.0), np.nextafter(F(1.0), F(2)))
    assert rr.decide(wide, one(1.0)) == dict(rolled=None, decided=False, tie=False, certain=False)
    assert rr.decide(wide, one(2.0)) == dict(rolled=True, decided=False, tie=False, certain=True)
    assert rr.determined(rr.mean_interval(np.zeros(0, F))) and np.isnan(rr.mean_interval(np.zeros(0, F))[0])


# ------------------------------------------------------------------------------------------------ the scenes' claims
def test_decoy_scenes_roll_back_and_keep_as_claimed():
    for name in ("decoy_N1024", "poses_N1024"):
        ex = expected(name)
        assert [r["rolled"] for r in ex] == rc.get(name)["rolled"], (name, [r["rolled"] for r in ex])
        assert not any(r["tie"] for r in ex)
    c, o = rc.get("decoy_N1024"), oracle("decoy_N1024")
    assert abs(o["e0"][0] - 0.2196) < 2e-4 and abs(o["e1"][0] - 0.2400) < 2e-4 and abs(o["e0"][2] - 0.1383) < 2e-4 and abs(o["e1"][2] - 0.1200) < 2e-4


def test_every_decoy_row_is_outside_the_gate_and_the_scene_fits_the_width():
    for side, specs in ((24, rc.CLEAR + rc.SECOND_DECOY + [(449, 576)]), (16, [(256, 256), (257, 256)]), (5, [(38, 25), (39, 25), (30, 10), (10, 25)])):
        for nA, nB in specs:
            a, c = rc.anchor_and_decoy(nA, nB, side)
            assert len(a) == nA + nB and len(c) == nA + side * side
            for shift in (0.0, -rc.SHIFT):                           # before and after the ICP's motion
                d = np.sqrt(mr.min_d2(a[nA:].astype(F) + np.array([shift, 0, 0], F), c.astype(F)))
                assert d.min() > rc.THRES * 2, (nA, nB, side, d.min())
    for name in rc.CASES:
        c = rc.get(name)
        N = c["S"].shape[1]
        assert all(n <= N and m <= N for n, m in rc.lens_of(c))
    assert all(nA + 576 <= 1024 for nA, _ in rc.CLEAR + rc.SECOND_DECOY)


def test_the_second_application_has_exact_ties_with_a_changed_pose():
    for name in ("second_decoy_N1024", "second_ragged_N512"):
        ex, o = expected(name), oracle(name)
        ties = [b for b, r in enumerate(ex) if r["decided"] and r["tie"] and not rr.same_bits(r["M"], o["init"][b])]
        assert ties, name
        assert all(ex[b]["rolled"] for b in ties)
    # the ragged batch: decisions that hang on a few float32 steps, both ways
    ex = expected("second_ragged_N512")
    near = [r for r in ex if abs(float(r["e1"][0]) - float(r["e0"][0])) <= 1e-5 * float(r["e0"][0])]
    assert len(near) >= 12 and {r["rolled"] for r in near} == {True, False}


def test_the_batch_that_never_stops():
    for m in rc.STOP_ITERATIONS:
        assert oracle(f"stop_{m}_N64")["iterations"] == m
    assert oracle("batch_B65_N64")["iterations"] <= 50


def test_empty_sides():
    c = rc.get("empty_N300")
    assert rc.lens_of(c)[:5] == [(200, 0), (0, 200), (0, 0), (1, 1), (1, 200)]
    ex = expected("empty_N300")
    assert ex[0]["rolled"] is True and ex[0]["decided"]                       # an empty destination: the initial pose
    assert ex[1]["rolled"] is False and ex[2]["rolled"] is False             # an empty source: 0 / 0, the ICP's pose is kept
    assert np.isnan(ex[1]["e0"][0]) and np.isnan(ex[2]["e1"][0])


def test_hist_batches_have_both_swap_states():
    for N in (300, 2049):
        S, D = rc.hist_batch(N)
        A, C, sw = rc.by_role(S, D)
        assert sw.sum() >= 6 and (~sw).sum() >= 6
        assert ((A[:, :, 3] > 0).sum(1) <= (C[:, :, 3] > 0).sum(1)).all()
        assert np.array_equal(A[~sw], S[~sw]) and np.array_equal(A[sw], D[sw]) and np.array_equal(C[sw], S[sw])


def test_a_swapped_pair_decides_differently_by_the_other_length():
    """found on the CPU, with the oracle's poses standing in: among the thousand near-ties at least one pair whose decision flips when
    its sums are divided by the fixed cloud's length; every pair is swapped and decided"""
    S, D = rc.length_sensitive_batch()
    A, C, sw = rc.by_role(S, D)
    assert sw.all() and set(rc.lens_of(dict(S=A, D=C))) == {(65, 113)}
    a = rp.default_args(max_points=128, thres_dist=rc.THRES)
    init = rp.estimate_init_pose(a, torch.from_numpy(A), torch.from_numpy(C))
    sol = rp.iterative_closest_point(rp.transform_points_batch(torch.from_numpy(A), init), torch.from_numpy(C), thres=rc.THRES,
                                     max_iterations=50, kabsch_dtype=torch.float64)
    ex = rr.expected(A, C, init.numpy(), sol.R.numpy(), sol.T.numpy(), swapped=sw)
    assert all(r["decided"] for r in ex)
    flips = [b for b, r in enumerate(ex) if rr.rule_with_the_other_length(r) != r["rolled"]]
    print("pairs that the other length decides differently:", flips)
    assert flips


# ------------------------------------------------------------------------------------------------ the paths
def test_paths_of_every_call_of_the_gpu_module():
    for name, variant, fin, kernel in rc.CALLS:
        c = rc.get(name)
        B, N = c["S"].shape[:2]
        kw = rc.call_args(name, variant)
        p = rr.check_path(B, N, rc.lens_of(c), kw.get("search", "auto"), kw.get("flags", ()), kw.get("arith", "fp64"),
                          kw["max_iterations"], kw.get("stop_mode", 0))
        assert (p["finish"], p["kernel"]) == (fin, kernel), (name, variant, p["finish"], p["kernel"])
        if "tokens" in c and p["dirs"] is not None:
            got = {f"{t}{s if t == 'full' else ''}" for t, s, _ in p["dirs"]}
            assert c["tokens"] <= got, (name, got)
    for name in rc.VARIANT_CASES:
        c = rc.get(name)
        B, N = c["S"].shape[:2]
        for variant, fin in rc.VARIANT_FINISH.items():
            kw = rc.call_args(name, variant)
            assert rr.finish(N, kw.get("search", "auto"), kw.get("flags", ()), kw.get("arith", "fp64"), kw["max_iterations"],
                             kw.get("stop_mode", 0)) == fin, (name, variant)
    # the staging case reads its keys from global memory; the others stage them in LDS
    assert [s for _, _, s in rr.check_path(2, 4112, rc.lens_of(rc.get("staging_N4112")))["dirs"]] == [False, True]
    assert rr.finish(1024, max_iterations=129) == "state" and rr.finish(63) == "unfused" and rr.finish(16385) == "unfused"

"""The roll-back on its own (rows a-8 / a-9): icpflow_apply_icp and icpflow_hist_icp against tests/rollback_restatement.py.

icpflow_icp runs the same ICP launch as icpflow_apply_icp and exports (R, T, iterations).  Given those floats the restatement says
which sixteen words every pair must return: the composed pose or the initial one, bit for bit, for every pair whose two means are
one float32 number each whatever order the library sums in (a DECIDED pair); for the pairs hist_icp swapped, the exact inverse of
that matrix within the derived bound (rollback_restatement.inverse_bound).  An undecided pair must still return one of the two
candidates; the whole module may meet ONE such pair, a second one is a failure.

Not one assertion here compares one variant of the library with another before it has compared both with the restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import match_eval_cases as mc                # noqa: E402
import rollback_cases as rc                  # noqa: E402
import rollback_device as dv                 # noqa: E402
import rollback_restatement as rr            # noqa: E402
from oracle import reference_path as rp      # noqa: E402

F = np.float32
TALLY = dict(pairs=0, decided=0, undecided=0, ties=0, tie_changed=0, rolled=0, kept=0, inverse_ratio=0.0, misrounded=0, inverted=0)
_D0, _E, _ICP = {}, {}, {}


def same_pose(a, b):
    """bit for bit; a NaN equal to a NaN whatever its payload (an empty cloud registers to NaN)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(((rr.bits(a) == rr.bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def restated(key, S, D, init, R, T, swapped=None):
    """rollback_restatement.expected, its distances under the initial poses computed once per batch and the whole of it once per
    ICP result (the variants of a call that leave the ICP alone share it)"""
    k0 = (key, init.tobytes())
    if k0 not in _D0:
        _D0[k0] = rr.init_distances(S, D, init)
    k1 = (key, init.tobytes(), R.tobytes(), T.tobytes())
    if k1 not in _E:
        _E[k1] = rr.expected(S, D, init, R, T, swapped=swapped, d0=_D0[k0])
    return _E[k1]


def compare(label, got, ex, init, count=True):
    """The call's sixteen words per pair against the restatement's records.  -> the records.  `count`: the pairs enter the module's
    tally (once per distinct ICP result, not once per variant that repeats it)."""
    for b, r in enumerate(ex):
        g = got[b]
        if r["swapped"]:
            continue                                     # (hist_icp's inverted pairs: compare_inverted)
        if r["certain"]:
            what = "rolled back: the initial pose" if r["rolled"] else "kept: compose(R, T of icpflow_icp, init)"
            assert same_pose(g, r["selected"]), (label, b, "ROLL-BACK" if same_pose(g, init[b]) or same_pose(g, r["M"]) else "POSE", what,
                                                 dict(e0=r["e0"], e1=r["e1"], n=r["n"], tie=r["tie"]), g, r["selected"])
        else:
            assert same_pose(g, init[b]) or same_pose(g, r["M"]), (label, b, "POSE: neither candidate", g)
    if count:
        tally(label, ex, init)
    return ex


def tally(label, ex, init):
    for b, r in enumerate(ex):
        TALLY["pairs"] += 1
        TALLY["decided" if r["decided"] else "undecided"] += 1
        TALLY["ties"] += int(r["tie"])
        TALLY["tie_changed"] += int(r["tie"] and not rr.same_bits(r["M"], init[b]))
        if r["rolled"] is not None:
            TALLY["rolled" if r["rolled"] else "kept"] += 1
    assert TALLY["undecided"] <= 1, (label, "more than one undecided pair in this module", TALLY)


def run_case(name, variant, stream=None, count=True):
    """icpflow_icp and icpflow_apply_icp on a case under a variant; the restatement from the former; the comparison
    -> (T_out, iterations, records)"""
    c = rc.get(name)
    kw = rc.call_args(name, variant)
    alias = kw.pop("alias", False)
    R, T, it_icp = dv.icp(c["S"], c["D"], c["init"], thres=rc.THRES, **kw)
    got, it = dv.apply_icp(c["S"], c["D"], c["init"], thres=rc.THRES, alias=alias, stream=stream, **kw)
    assert it == it_icp, (name, variant, "ICP: the two entry points count different iterations", it, it_icp)
    if "iterations" in c and variant == "default":
        assert it == c["iterations"], (name, "the batch was to run to the cap", it)
    ex = restated((name, kw.get("arith"), kw["max_iterations"], kw.get("stop_mode", 0)), c["S"], c["D"], c["init"], R, T)
    compare(f"{name}/{variant}", got, ex, c["init"], count)
    _ICP[(name, variant)] = (R, T)
    return got, it, ex


# ------------------------------------------------------------------------------------------------ 1. apply_icp = the restatement
@pytest.mark.parametrize("name,variant", [(n, v) for n, v, _, _ in rc.CALLS], ids=[f"{n}-{v}" for n, v, _, _ in rc.CALLS])
def test_apply_icp_equals_the_restatement(name, variant):
    """every scene, initial pose, width and batch size; the path of each call is pinned by tests/test_rollback_restatement.py"""
    _, _, ex = run_case(name, variant, count=variant == "default" or not any(n == name and v == "default" for n, v, _, _ in rc.CALLS))
    c = rc.get(name)
    if "rolled" in c:
        assert [r["rolled"] for r in ex] == c["rolled"], (name, [r["rolled"] for r in ex])
    print(f"{name}/{variant}: {len(ex)} pairs, decided {sum(r['decided'] for r in ex)}, ties {sum(r['tie'] for r in ex)}, "
          f"rolled back {sum(r['rolled'] is True for r in ex)}, kept {sum(r['rolled'] is False for r in ex)}")


def test_the_two_entry_points_run_the_same_icp():
    """Under the identity as initial pose the composition changes nothing (products by 0 and 1), so a kept pair returns the ICP's own
    [[R^T, T], [0 0 0 1]]: icpflow_apply_icp's ICP is icpflow_icp's, bit for bit, without compose_kernel's arithmetic in between."""
    c = rc.get("decoy_N1024")
    pairs = [rc.anchor_and_decoy(nA, nB) for nA, nB in rc.CLEAR]
    S, D = rc.sc.batch([(a.astype(F), d.astype(F)) for a, d in pairs], 1024)
    I = np.stack([np.eye(4, dtype=F)] * 4)
    R, T, it_icp = dv.icp(S, D, I, thres=rc.THRES)
    got, it = dv.apply_icp(S, D, I, thres=rc.THRES)
    assert it == it_icp
    kept = 0
    for b in range(4):
        A = np.eye(4, dtype=F)
        A[:3, :3], A[:3, 3] = R[b].T, T[b]
        assert np.array_equal(rr.compose(R[b], T[b], I[b]), A)
        if not same_pose(got[b], I[b]):
            assert np.array_equal(got[b], A), ("ICP: icpflow_apply_icp's pose is not icpflow_icp's", b, got[b], A)
            kept += 1
    assert kept == 2 and c["rolled"] == [same_pose(got[b], I[b]) for b in range(4)]


# ------------------------------------------------------------------------------------------------ 2. the finishes and their switches
@pytest.mark.parametrize("name", rc.VARIANT_CASES)
def test_the_three_finishes_leave_the_same_words(name):
    """Every variant against its OWN restatement (run_case), from the ICP pose icpflow_icp exports under the same switches.  Then the
    variants among each other: a switch that leaves the ICP launch alone (no_speculative, no_check_sweep, the aliased output) must
    return the default's sixteen words per pair.  SCAN and GRID replace the ICP's search as well: they visit the source rows in the
    same order and must agree with each other bit for bit; the sorted sweep adds the same fp64 moments in sorted order, so its ICP
    pose may differ from theirs in the last float32 bit (tests/test_gpu_parity.py test_search_modes_agree) -- where the exported
    (R, T) ARE the default's bits, the words must be the default's too, and the pairs where they are not are printed."""
    base, it0, _ = run_case(name, "default", count=False)
    R0, T0 = _ICP[(name, "default")]
    outs = {}
    for variant in rc.VARIANTS:
        if variant == "default":
            continue
        got, it, _ = run_case(name, variant, count=variant in ("one_iteration", "per_pair", "fp32_reference"))
        outs[variant] = (got, it)
        if variant not in rc.SAME_AS_DEFAULT:
            continue
        R, T = _ICP[(name, variant)]
        same_icp = [b for b in range(len(base)) if rr.same_bits(R[b], R0[b]) and rr.same_bits(T[b], T0[b])]
        if variant not in ("scan", "grid"):
            assert len(same_icp) == len(base), (name, variant, "ICP: the exported pose differs from the default call's")
        else:
            print(f"{name}/{variant}: the ICP pose is the sorted sweep's bit for bit on {len(same_icp)} of {len(base)} pairs")
        assert it == it0, (name, variant, it, it0)
        for b in same_icp:
            assert same_pose(got[b], base[b]), (name, variant, b, "differs from the default call", got[b], base[b])
    (Rs, Ts), (Rg, Tg) = _ICP[(name, "scan")], _ICP[(name, "grid")]
    assert outs["scan"][1] == outs["grid"][1]
    for b in range(len(base)):
        if rr.same_bits(Rs[b], Rg[b]) and rr.same_bits(Ts[b], Tg[b]):
            assert same_pose(outs["scan"][0][b], outs["grid"][0][b]), (name, b, "scan and grid: the same ICP pose, other words")


# ------------------------------------------------------------------------------------------------ 3. the exact tie
@pytest.mark.parametrize("name", ["second_decoy_N1024", "second_ragged_N512"])
def test_the_exact_tie_returns_the_initial_pose(name):
    """The second application: the initial poses are the library's own results of a first call.  A pair whose restated means are the
    SAME float32 number while the composed pose differs from the initial one shows `>=`: it returns the initial pose."""
    c = rc.get(name)
    first, _ = dv.apply_icp(c["S"], c["D"], c["init"], thres=rc.THRES)
    assert np.isfinite(first).all()
    R, T, it_icp = dv.icp(c["S"], c["D"], first, thres=rc.THRES)
    ex = restated((name, "second"), c["S"], c["D"], first, R, T)
    ties = [b for b, r in enumerate(ex) if r["decided"] and r["tie"] and not rr.same_bits(r["M"], first[b])]
    for flags in ((), ("no_speculative",), ("no_check_sweep",)):
        got, it = dv.apply_icp(c["S"], c["D"], first, thres=rc.THRES, flags=flags)
        assert it == it_icp
        compare(f"{name}/second{flags}", got, ex, first, count=flags == ())
        for b in ties:
            assert rr.same_bits(got[b], first[b]) and not rr.same_bits(got[b], ex[b]["M"]), (name, flags, b)
    near = sum(abs(float(r["e1"][0]) - float(r["e0"][0])) <= 1e-5 * float(r["e0"][0]) for r in ex)
    print(f"{name}: exact ties with a changed pose {ties}, pairs within 1e-5 relative {near} of {len(ex)}, rolled back "
          f"{sum(r['rolled'] is True for r in ex)}, kept {sum(r['rolled'] is False for r in ex)}")
    if name == "second_decoy_N1024":
        assert ties, (name, "the scene has lost its exact tie", [(r["e0"], r["e1"]) for r in ex])
    else:
        assert near >= 12


# ------------------------------------------------------------------------------------------------ empty sides
@pytest.mark.parametrize("name", ["empty_N300", "empty_N2049"])
def test_empty_sides(name):
    c = rc.get(name)
    lens = rc.lens_of(c)
    outs = {}
    for variant in ("default", "no_speculative", "no_check_sweep", "scan"):
        outs[variant], _, ex = run_case(name, variant, count=variant == "default")
        for b, (n, m) in enumerate(lens):
            if n > 0 and m == 0:        # +inf >= +inf (scans), 0 >= 0 (sweeps): the initial pose
                assert rr.same_bits(outs[variant][b], c["init"][b]), (name, variant, b, outs[variant][b])
    for variant, got in outs.items():
        assert same_pose(got, outs["default"]), (name, variant)
    a = rp.default_args(max_points=c["S"].shape[1], thres_dist=rc.THRES)
    with np.errstate(all="ignore"):
        want = rp.apply_icp(a, torch.from_numpy(c["S"]), torch.from_numpy(c["D"]), torch.from_numpy(c["init"]), max_iterations=50,
                            kabsch_dtype=torch.float64).numpy()
    for b, (n, m) in enumerate(lens):
        if n == 0:                      # 0 / 0 on both sides: the ICP's pose is kept -- what the reference returns for the pair
            g = outs["default"][b]
            assert np.array_equal(np.isnan(g), np.isnan(want[b])) and np.allclose(g, want[b], atol=1e-4, equal_nan=True), (name, b, g, want[b])


# ------------------------------------------------------------------------------------------------ 4. hist_icp, unfolded by role
HIST_FLAGS = [(), ("no_check_reuse",), ("no_score_prune",), ("no_front_roles",), ("no_side_stream",)]


def unfolded(key, S, D):
    """utils_match.py:138-157 by role: the clouds of the pairs with n_src > n_dst exchanged on the host, the initial poses from
    icpflow_estimate_init_pose, (R, T) from icpflow_icp -> (records, initial poses, swapped, iterations)"""
    A, C, sw = rc.by_role(S, D)
    init = dv.estimate_init_pose(A, C, thres=rc.THRES)
    R, T, it = dv.icp(A, C, init, thres=rc.THRES)
    return restated(key, A, C, init, R, T, swapped=sw), init, sw, it


def compare_inverted(label, got, ex, count):
    for b, r in enumerate(ex):
        if not r["swapped"]:
            continue
        cands = [r["selected"]] if r["certain"] else [r["M"], None]
        oks = []
        for P in cands:
            if P is None:
                continue
            ok, worst, mis = rr.check_inverse(got[b], P)
            oks.append(ok)
            if ok and count:
                TALLY["inverse_ratio"] = max(TALLY["inverse_ratio"], worst)
                TALLY["misrounded"] += mis
                TALLY["inverted"] += 1
        assert any(oks), (label, b, "INVERSE: not within the bound of the exact inverse of the selected pose", got[b], r["selected"])


@pytest.mark.parametrize("N", [300, 2049])
def test_hist_icp_unfolded_by_role(N):
    S, D = rc.hist_batch(N)
    ex, init, sw, it_icp = unfolded(("hist", N), S, D)
    for side in (False, True):
        rolled = [b for b, r in enumerate(ex) if r["swapped"] == side and r["rolled"] is True]
        kept = [b for b, r in enumerate(ex) if r["swapped"] == side and r["rolled"] is False]
        assert len(rolled) >= 2 and len(kept) >= 2, (N, "swapped" if side else "not swapped", rolled, kept)
    flips = [b for b, r in enumerate(ex) if r["swapped"] and r["decided"] and rr.rule_with_the_other_length(r) != r["rolled"]]
    for flags in HIST_FLAGS:
        got, it = dv.hist_icp(S, D, thres=rc.THRES, flags=flags)
        assert it == it_icp, (N, flags, "ICP: hist_icp and icpflow_icp count different iterations", it, it_icp)
        # an inverted pair whose selected pose is not certain cannot be told by its words: the restatement needs the choice
        for b, r in enumerate(ex):
            if r["swapped"] and not r["certain"]:
                r["selected"] = r["M"] if rr.check_inverse(got[b], r["M"])[0] else init[b]
                r["certain"] = True
        compare(f"hist_icp N={N} {flags}", got, ex, init, count=flags == ())
        compare_inverted(f"hist_icp N={N} {flags}", got, ex, count=flags == ())
    print(f"hist_icp N={N}: swapped {int(sw.sum())} of {len(sw)}, rolled back {sum(r['rolled'] is True for r in ex)}, kept "
          f"{sum(r['rolled'] is False for r in ex)}, pairs whose decision the other length would flip {flips}")


def test_hist_icp_divides_by_the_moving_clouds_length():
    """rollback_cases.length_sensitive_batch: a thousand swapped near-ties.  The restated means divide by the moving cloud's length --
    lenC for a swapped pair --; at least one pair of the batch decides differently by the other length, and returns what the right
    one says."""
    S, D = rc.length_sensitive_batch()
    ex, init, sw, it_icp = unfolded(("hist_len", 128), S, D)
    assert sw.all() and all(r["decided"] for r in ex)
    flips = [b for b, r in enumerate(ex) if rr.rule_with_the_other_length(r) != r["rolled"]]
    got, it = dv.hist_icp(S, D, thres=rc.THRES)
    assert it == it_icp
    compare_inverted("hist_icp near-ties", got, ex, count=False)
    print(f"hist_icp near-ties: rolled back {sum(r['rolled'] for r in ex)} of {len(ex)}, exact ties {sum(r['tie'] for r in ex)}, "
          f"pairs that the other length decides differently {flips}")
    assert flips, "the batch has lost the pairs that tell the two lengths apart"


def test_hist_icp_above_the_direction_keys():
    """the ragged batch of the icpflow_hist_icp_eval test at N = 2049: two thin boxes turned by 45 degrees, whose fixed cloud the
    sort orders along a direction key"""
    S, D = mc.hist_icp_eval_batch(2049)
    ex, init, sw, it_icp = unfolded(("hist_dir", 2049), S, D)
    got, it = dv.hist_icp(S, D, thres=rc.THRES)
    assert it == it_icp
    compare("hist_icp thin boxes", got, ex, init)
    compare_inverted("hist_icp thin boxes", got, ex, count=True)


# ------------------------------------------------------------------------------------------------ 5. reruns, a second stream
def test_reruns_and_a_second_stream_are_bit_identical():
    c = rc.get("windows_N2049")
    base, it0, _ = run_case("windows_N2049", "default", count=False)
    again, it1 = dv.apply_icp(c["S"], c["D"], c["init"], thres=rc.THRES)
    side = torch.cuda.Stream()
    other, it2, _ = run_case("windows_N2049", "default", stream=side, count=False)
    assert it0 == it1 == it2 and rr.same_bits(base, again) and rr.same_bits(base, other)
    S, D = rc.hist_batch(300)
    h0, i0 = dv.hist_icp(S, D, thres=rc.THRES)
    h1, i1 = dv.hist_icp(S, D, thres=rc.THRES)
    h2, i2 = dv.hist_icp(S, D, thres=rc.THRES, stream=side)
    assert i0 == i1 == i2 and rr.same_bits(h0, h1) and rr.same_bits(h0, h2)


# ------------------------------------------------------------------------------------------------ the module's tally
def test_zz_the_modules_tally():
    """at most one undecided pair in the whole module (asserted as the tally grows, and here); the figures of COVERAGE.md"""
    print("roll-back tally:", TALLY)
    assert TALLY["undecided"] <= 1, TALLY

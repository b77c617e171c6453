"""CPU-only: tests/sort_restatement.py against exact rationals and Python's own sort, its key choice on clouds whose code one can
say aloud, and the conditions on the inputs of tests/test_gpu_sorts.py (tests/sort_cases.py) -- conditions, not measurements."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_cases as sc          # noqa: E402
import sort_restatement as sr    # noqa: E402

F = np.float32


def round_f32(x):
    """the float32 nearest to the Fraction x, ties to even, denormals included (|x| far below float32's overflow)"""
    if x == 0:
        return F(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                   # 2^e <= a < 2^(e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)       # the spacing of float32 there
    n = a / q
    k = n.numerator // n.denominator
    rest = n - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    v = float(k * q)                             # exact: k < 2^25, q a power of two
    return F(-v if x < 0 else v)


def _triples(n, seed=5):
    rng = np.random.default_rng(seed)
    bits = lambda m: rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32).view(F)    # noqa: E731
    third = n // 5
    a, b, c = [], [], []
    # any finite bit patterns whose product stays far from overflow
    x, y, z = bits(4 * third), bits(4 * third), bits(4 * third)
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (np.abs(x) < 1e18) & (np.abs(y) < 1e18) & (np.abs(z) < 1e36)
    a.append(x[ok][:third]); b.append(y[ok][:third]); c.append(z[ok][:third])
    # the sizes the keys have: coordinates times direction cosines
    a.append(rng.choice([0.9238795, 0.3826834, 0.7071067, -0.3826834], third).astype(F))
    b.append(rng.uniform(-3000, 3000, third).astype(F))
    c.append(rng.uniform(-3000, 3000, third).astype(F))
    # cancellation: c = -fl(a b), and one ulp beside it
    x, y = rng.uniform(-100, 100, third).astype(F), rng.uniform(-100, 100, third).astype(F)
    p = -(x * y)
    a.append(x); b.append(y); c.append(np.where(rng.random(third) < 0.5, p, np.nextafter(p, F(np.inf))).astype(F))
    # halfway cases: a b = m 2^-24 with m odd next to c = 1 (or 2^k): the exact sum lies exactly between two float32s, or one bit off it
    # (for half of them a b itself is odd in [2^24, 2^25) -- exactly between two float32s -- and c = +-2^-40 pushes the exact sum off the
    # tie by less than float64 can hold beside 2^24: an evaluation in float64 rounds back onto the tie, and then to even)
    m = (2 * rng.integers(0, 1 << 22, third) + 1).astype(F)
    y = np.where(rng.random(third) < 0.5, F(2.0) ** -24, F(2.0) ** -24 * (F(1) + F(2.0) ** -23)).astype(F)
    z = (F(2.0) ** rng.integers(0, 3, third)).astype(F) * rng.choice([1, -1], third).astype(F)
    odd = (2 * rng.integers(2048, 2895, (2, third)) + 1).astype(F)
    tie = rng.random(third) < 0.5
    a.append(np.where(tie, odd[0], m).astype(F)); b.append(np.where(tie, odd[1], y).astype(F))
    c.append(np.where(tie, rng.choice([1, -1], third) * 2.0 ** -40, z).astype(F))
    # denormal results and operands
    x = (rng.uniform(-1, 1, third) * 1e-20).astype(F)
    y = (rng.uniform(-1, 1, third) * 1e-20).astype(F)
    z = rng.integers(-40, 40, third).astype(np.int32).view(F)      # the smallest denormals; negative ints: huge patterns, filtered
    z = np.where(np.isfinite(z) & (np.abs(z) < 1e-30), z, F(1e-45)).astype(F)
    a.append(x); b.append(y); c.append(z)
    return np.concatenate(a), np.concatenate(b), np.concatenate(c)


def test_fma32_equals_the_exact_rational_result():
    a, b, c = _triples(100_000)
    assert len(a) >= 100_000 - 5
    got = sr.fma32(a, b, c)
    want = np.array([round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], F)
    # (-0.0 and +0.0: the rational zero has no sign; the library canonicalises every key with + 0.0f)
    bad = np.flatnonzero(sr.canonical(got).view(np.uint32) != sr.canonical(want).view(np.uint32))
    assert len(bad) == 0, (len(bad), a[bad[:3]], b[bad[:3]], c[bad[:3]], got[bad[:3]], want[bad[:3]])
    # ... and the emulation is not a plain float64 evaluation rounded twice: some of the halfway triples tell the two apart
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    assert (twice != got).sum() > 0


def test_order_equals_pythons_sort_on_key_row_tuples():
    rng = np.random.default_rng(3)
    for keys in (rng.integers(-3, 4, 5000).astype(F) * F(0.5),
                 np.array([0.0, -0.0, 1e-45, -1e-45, -0.0, 0.0, 1e-45, -1e-40, 3000.0002, -1e6, 1e6, 999999.94], F),
                 rng.normal(0, 1, 4097).astype(F), np.zeros(2049, F), np.zeros(0, F)):
        want = [r for _, r in sorted((float(k) + 0.0, r) for r, k in enumerate(keys))]
        assert sr.order(keys).tolist() == want
    assert sr.canonical(np.array([-0.0], F)).view(np.uint32)[0] == 0


def test_lengths_roles_and_the_strict_swap():
    a, b = sc.cloud(np.zeros((5, 3)), 8), sc.cloud(np.zeros((5, 3)), 8)
    assert sr.roles(a, b)[:3] == (5, 5, 0)                    # equal lengths: no swap
    assert sr.roles(sc.cloud(np.zeros((6, 3)), 8), b)[:3] == (6, 5, 1)
    assert sr.roles(b, sc.cloud(np.zeros((6, 3)), 8))[:3] == (5, 6, 0)
    assert sr.roles(sc.cloud(np.zeros((0, 3)), 8), b)[:3] == (0, 5, 0)


def test_codes_one_can_say_aloud():
    fixed_n, nx = 2000, 2000
    assert sr.choose_code(sc.cube(fixed_n), nx)[0] == 0
    assert sr.choose_code(sc.box_e1_eq_e2(fixed_n), nx)[0] == 1
    assert sr.choose_code(sc.box_e1_eq_e2(fixed_n)[:, [1, 2, 0]], nx)[0] == 0         # e0 = e1 > e2
    assert sr.choose_code(sc.box_e1_eq_e2(fixed_n)[:, [1, 0, 2]], nx)[0] == 0         # e0 = e2 > e1
    code, info = sr.choose_code(sc.thin_box(2000, 45.0), nx)
    s = info["scores"]
    print(f"thin box turned 45 deg, 2000 rows: code {code}, legacy {info['legacy']}, scores {s}, margin {info['margin']} "
          f"({info['margin'] / s[info['legacy']]:.3f} s_legacy), gap {info['gap']} ({info['gap'] / s[info['legacy']]:.3f} s_legacy)")
    assert code == 4 and info["margin"] >= 0.05 * s[info["legacy"]] and info["gap"] >= 0.05 * s[info["legacy"]]
    code, info = sr.choose_code(sc.thin_box(2000, 0.0), nx)
    assert code == info["legacy"] == 0 and -info["margin"] >= 0.05 * info["scores"][0]
    # the thresholds: a direction needs ny >= 1025 and nx >= 512, and the permission of the call
    assert sr.choose_code(sc.thin_box(1025, 45.0), 512)[0] == 4
    assert sr.choose_code(sc.thin_box(1024, 45.0), 512)[0] <= 2
    assert sr.choose_code(sc.thin_box(1025, 45.0), 511)[0] <= 2
    assert sr.choose_code(sc.thin_box(1025, 45.0), 512, dir_keys=False)[0] <= 2


def test_direction_keys_are_one_product_and_one_fma():
    p = sc.thin_box(500, 45.0)
    for code, (ux, uy) in sr.SORT_DIRS.items():
        want = np.array([round_f32(Fraction(float(uy)) * Fraction(float(y)) + Fraction(float(ux * x))) for x, y in p[:, :2]], F)
        assert np.array_equal(sr.axis_key(code, p), want)
        assert float(ux) ** 2 + float(uy) ** 2 <= 1.0                                    # rounded towards zero: |u| <= 1
    for code in range(3):
        assert np.array_equal(sr.axis_key(code, p), p[:, code])


def _tied_rows(keys):
    _, inv, cnt = np.unique(sr.canonical(keys), return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def test_the_gpu_cases_are_the_cases_their_names_claim():
    for N in (2048, 4096, 4097, 8200):
        S, D, names, want = sc.key_choice_batch(N)
        for b, (name, w) in enumerate(zip(names, want)):
            r = sr.axis_sorted_pair(S[b], D[b])
            i = r["info"]
            if w == "below":
                assert i["scores"] is None and r["code"] <= 2, (N, name)
                continue
            sl = i["scores"][i["legacy"]]
            print(f"N {N} {name}: code {r['code']} legacy {i['legacy']} margin {i['margin'] / sl:+.3f} s_legacy gap {i['gap'] / sl:.3f} s_legacy")
            if w == "direction":      # chosen: both the decision against the legacy code and the pick among the others stand clear
                assert r["code"] == 4 and i["margin"] >= 0.05 * sl and i["gap"] >= 0.05 * sl, (N, name, i)
            else:                     # kept: only the best of the OTHER codes against nine tenths of the legacy score decides
                assert r["code"] == i["legacy"] and -i["margin"] >= 0.05 * sl, (N, name, i)
        assert r["swap"] == 1         # (the last pair: the src cloud is the fixed one)
    for N in (4096, 8200):
        S, D, names, ties = sc.ties_batch(N)
        for b, (name, t) in enumerate(zip(names, ties)):
            r = sr.axis_sorted_pair(S[b], D[b], swap_allowed=False)
            n = r["ny"]
            kx, kz = sr.axis_key(r["code"], D[b, :n, :3]), D[b, :n, 2]
            tx, tz = _tied_rows(kx), _tied_rows(kz)
            print(f"N {N} {name}: code {r['code']}, {n} rows, {tx} tied under the axis key, {tz} under z")
            assert tx >= t and tz >= t, (N, name, tx, tz, t)
            if name != "duplicates":
                assert r["code"] == 0, name
        b = names.index("signed_zeros")
        x = D[b, :, 0]
        assert ((x == 0) & np.signbit(x)).sum() > 100 and ((x == 0) & ~np.signbit(x)).sum() > 100
        assert np.abs(np.diff(np.signbit(x[x == 0]).astype(int))).sum() > 100          # interleaved in row order
        b = names.index("denormals")
        x = D[b, :sr.length(D[b]), 0]
        assert ((x != 0) & (np.abs(x) < np.finfo(F).tiny)).sum() > 1000
        b = names.index("three_keys")
        assert len(np.unique(D[b, :sr.length(D[b]), 0])) == 3
        if N > 4096:      # runs of equal keys cross the 2048-row chunk seams: every chunk holds all three keys
            assert all(len(np.unique(D[b, c:min(c + 2048, sr.length(D[b])), 0])) == 3 for c in (0, 2048, 4096))
    h = sc.WIDE_EZ[-1] - sc.WIDE_EZ[0]
    assert h == F(0.25)
    for N in (4096, 4097, 8200):
        S, D, names, want = sc.wide_batch(N)
        for b, (name, w) in enumerate(zip(names, want)):
            rec = sr.vote_key_record(S[b], D[b], h)
            assert rec[:2] == w, (N, name, rec)
            if "slab" in name or name in ("wall_x_4097_rows", "wall_y", "z_range_below_250_h"):
                q = sr.vote_slab(rec, S[b, :sr.length(S[b]), :3])
                on_border = int((q == np.floor(q)).sum())
                assert rec[0] == 1 and on_border >= 300, (N, name, on_border)
    for N in (1024, 1025, 4096, 4097, 8200):
        S, D = sc.seam_batch(N)
        got = sorted({sr.length(c) for c in list(S) + list(D)})
        listed = [c for c in (sc.SINGLE_COUNTS if N <= 4096 else sc.CHUNKED_COUNTS) if c <= N] + [N]
        assert got == sorted(set(listed)), (N, got)
        sw = [sr.roles(s, d)[2] and sr.length(d) > 0 for s, d in zip(S, D)]      # (swapped roles with rows on both sides)
        eq = [sr.length(s) == sr.length(d) for s, d in zip(S, D)]
        assert sum(sw) == 2 and sum(eq) == 2


def test_the_layout_entry_refuses_bad_arguments():
    """icpflow_selftest_workspace_layout is host only: a wrong count, a null pointer or a non-positive size is ICPFLOW_E_ARG; the
    offsets are distinct multiples of 256 inside the workspace."""
    import ctypes
    from icp_flow_amd import _lib
    off = (ctypes.c_size_t * 11)()
    L = _lib._L
    assert L.icpflow_selftest_workspace_layout(4, 1024, 41, 41, 3, off, 10) == -1 and b"count" in L.icpflow_last_error()
    assert L.icpflow_selftest_workspace_layout(4, 1024, 41, 41, 3, None, 11) == -1
    assert L.icpflow_selftest_workspace_layout(0, 1024, 41, 41, 3, off, 11) == -1
    assert L.icpflow_selftest_workspace_layout(4, 1024, 41, 41, 3, off, 11) == 0
    o = list(off)
    assert all(x % 256 == 0 for x in o) and len(set(o)) == 11 and max(o) < L.icpflow_workspace_bytes(4, 1024, 41, 41, 3)

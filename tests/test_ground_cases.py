"""CPU proof that every input of tests/ground_cases.py is the case its name claims, in numbers that are printed before they are
asserted.  For every case: all patches of at least num_min_pts rows are determined (ground_restatement.determined) at the case's
own parameters, no row is left out of the comparison, and no row but the ones a case puts ON a border is within 1e-9 of a bin of
one.  For every parameter case: the restatement at the DEFAULT value gives another code, revert outcome or ground count and at
least 20 other labels, so a library that ignored the parameter cannot pass.  (num_min_pts = 1 is the one exception, and it is
one of arithmetic: the only patches that 1 admits and 10 does not, without the rank-deficient ones of 2 to 9 rows, have ONE row,
whose plane is NaN and whose row stays non-ground either way.  It bites on the codes and means of 21 such patches.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_cases as gc            # noqa: E402
import ground_restatement as gr      # noqa: E402


@pytest.mark.parametrize("name", sorted(gc.NAMES))
def test_every_patch_is_determined_and_no_row_is_left_out(name):
    case = gc.get(name)
    res, par = case["res"], case["params"]
    big = res["table"][:, 0] >= par.num_min_pts
    det, keep = gr.determined(res, par), gr.rows_to_compare(res, par)
    rows = np.ones(len(case["pts"]), dtype=bool)
    if "special" in case.get("parts", {}):
        rows[case["parts"]["special"]] = False
    border = res["border"][rows].min() if rows.any() else np.inf
    print(f"{name}: {case['claim']}; rows {len(keep)}, patches of >= {par.num_min_pts} rows {int(big.sum())}, undetermined {int((big & ~det).sum())}, "
          f"smallest margin {res['margin'][big].min():.3e}, smallest gap {res['gap'][big].min():.3e}, rows left out {int((~keep).sum())}, "
          f"nearest border {border:.3e} bins")
    assert big.sum() >= 1 and border > 1e-9
    if gc.NAMES[name] == "E":                  # the two named degenerate patches, one by one, and nothing else
        assert set(np.flatnonzero(big & ~det)) == set(case["leave_out"]) and len(case["leave_out"]) == (2 if name == "exact_lattices" else 0)
        assert np.array_equal(~keep, np.isin(res["patch"], case["leave_out"]))
    else:
        assert (det == big).all() and keep.all()


# ---- P ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.GROUPS["P"]))
def test_parameter_case_bites(name):
    case = gc.get(name)
    res, pts = case["res"], case["pts"]
    other = gr.segment(pts, case["default"])
    t, u = res["table"], other["table"]
    patches = int(((t[:, 12] != u[:, 12]) | (t[:, 13] != u[:, 13]) | (t[:, 1] != u[:, 1])).sum())
    labels = int((res["nonground"] != other["nonground"]).sum())
    print(f"{name}: at the default value {patches} patches have another code, revert outcome or ground count, {labels} rows another label")
    assert patches >= 1
    if name == "num_min_pts[1]":
        single = np.flatnonzero(t[:, 0] == 1)
        assert len(single) >= 20 and (t[single, 12] == gr.NOT_UPRIGHT).all() and (u[single, 12] == gr.TOO_FEW).all()
        assert np.isnan(t[single, 5:12]).all() and (t[single, 1] == 0).all() and np.isfinite(t[single, 2:5]).all() and labels == 0
        assert not ((t[:, 0] >= 2) & (t[:, 0] <= 9)).any()
    else:
        assert labels >= 20


def test_num_min_pts_30_has_patches_of_29_and_30():
    t = gc.get("num_min_pts[30]")["res"]["table"]
    assert (t[:, 0] == 29).sum() == 1 and (t[:, 0] == 30).sum() >= 1
    assert (t[t[:, 0] == 29, 12] == gr.TOO_FEW).all() and (t[t[:, 0] == 30, 12] != gr.TOO_FEW).all()


def test_num_lpr_64_has_a_patch_with_fewer_candidates():
    case = gc.get("num_lpr[64]")
    rows = case["parts"]["most_below"]
    z = case["pts"][rows, 2].astype(np.float64)
    left = int((~(z < case["params"].skip_below)).sum())
    print("most_below: candidates after the zone-0 skip", left)
    assert len(set(case["res"]["patch"][rows])) == 1 and case["res"]["patch"][rows[0]] < 32 and 0 < left < 64


@pytest.mark.parametrize("name", ["adaptive_seed_selection_margin[-1.0]", "adaptive_seed_selection_margin[-2.0]", "adaptive_seed_selection_margin[0.0]"])
def test_margin_cases_have_patches_partly_and_wholly_below(name):
    case = gc.get(name)
    pid, z, skip = case["res"]["patch"], case["pts"][:, 2].astype(np.float64), case["params"].skip_below
    some = all_ = 0
    for p in range(32):
        zz = z[pid == p]
        if len(zz) >= 10:
            below = int((zz < skip).sum())
            some += 0 < below < len(zz)
            all_ += below == len(zz)
    print(f"{name}: skip below {skip:.4f}: zone-0 patches partly below {some}, wholly below {all_}")
    assert some >= 1 and all_ >= 1


def test_uprightness_cases_have_ramps_on_both_sides_near_and_far():
    for name, v in (("uprightness_thr[0.5]", 0.5), ("uprightness_thr[0.9]", 0.9)):
        case = gc.get(name)
        t = case["res"]["table"]
        for where in ("near", "far"):
            nz = {a: t[case["res"]["patch"][case["parts"][f"{where}{a}"][0]], 7] for a in (20, 35, 52, 65)}
            # (a near ramp that is not upright is taken away by R-VPF; what is left has another plane, so the far ones show the angles)
            print(name, where, {a: round(float(x), 4) for a, x in nz.items()})
        far = [t[case["res"]["patch"][case["parts"][f"far{a}"][0]], 7] for a in (20, 35, 52, 65)]
        assert np.allclose(far, np.cos(np.radians([20, 35, 52, 65])), atol=2e-3)
        assert any(x > v for x in far) and any(x < v for x in far) and any((x > v) != (x > 0.707) for x in far)
        near_codes = [int(t[case["res"]["patch"][case["parts"][f"near{a}"][0]], 14] > 0) for a in (20, 35, 52, 65)]
        assert 0 < sum(near_codes) < 4                                    # R-VPF took some near ramps and left others


@pytest.mark.parametrize("name", ["ranges_dyadic", "ranges_2p7_80"])
def test_ranges_cases_put_rows_on_the_borders(name):
    case = gc.get(name)
    par, res, sp = case["params"], case["res"], case["parts"]["special"]
    xy = case["pts"][sp, 0:2].astype(np.float64)
    r = np.abs(xy).max(axis=1)
    assert (np.abs(xy).min(axis=1) == 0).all()                            # on an axis: r = |x| or |y|, exactly
    edges = np.asarray((par.min_range, par.max_range) + par.lo[1:])
    pid = res["patch"][sp]
    if name == "ranges_dyadic":
        borders = np.asarray([par.lo[k] + j * par.ring_size[k] for k in range(4) for j in range(gr.RINGS[k])] + [par.max_range])
        assert par.lo == (2.0, 10.0, 18.0, 34.0) and par.ring_size == (4.0, 2.0, 4.0, 8.0)
        assert sorted(set(r)) == sorted(borders) and len(sp) == 4 * 15 and (res["border"][sp] < 1e-12).all()
        assert (pid[r == 2.0] == -1).all() and (pid[r == 66.0] >= gr.patch_index(3, 3, 0)).all()
        for k in (1, 2, 3):                                               # a zone border belongs to the outer zone, ring 0
            zone, ring, _ = gc.patch_zrs(pid[r == par.lo[k]])
            assert (zone == k).all() and (ring == 0).all()
    else:
        for e in edges:                                                   # float32 neighbours of the edge on both sides
            near = np.unique(r[np.abs(r - e) < 1e-4])
            print(f"{name}: edge {e!r}: rows at r - edge = {[float(x - e) for x in near]}")
            below, above = near[near < e], near[near > e]
            assert len(below) >= 1 and len(above) >= 1
            assert below.max() == np.float64(np.nextafter(np.float32(above.min()), np.float32(-np.inf))) or e in near
        assert (pid[(r > par.min_range) & (r <= par.max_range)] >= 0).all() and (pid[(r <= par.min_range) | (r > par.max_range)] == -1).all()
        for k in (1, 2, 3):
            zone, _, _ = gc.patch_zrs(pid[(np.abs(r - par.lo[k]) < 1e-4) & (r < par.lo[k])])
            assert (zone == k - 1).all()
            zone, _, _ = gc.patch_zrs(pid[(np.abs(r - par.lo[k]) < 1e-4) & (r >= par.lo[k])])
            assert (zone == k).all()
    inside = pid[pid >= 0]
    assert (res["table"][inside, 0] >= 30).all()                          # a patch of rows on either side of each border
    assert len(set(inside)) >= (4 * 13 if name == "ranges_dyadic" else 4 * 8)
    for zone in range(4):                                                 # the patches on both sides of every axis, in every ring
        S = gr.SECTORS[zone]
        for ring in range(gr.RINGS[zone]):
            for sector in (S - 1, 0, S // 4 - 1, S // 4, S // 2 - 1, S // 2, (3 * S) // 4 - 1, (3 * S) // 4):
                assert res["table"][gr.patch_index(zone, ring, sector), 0] >= 30
    assert not res["nonground"][sp[pid >= 0]].any() and res["nonground"][sp[pid < 0]].all()


# ---- N ----------------------------------------------------------------------------------------------------------------------
def test_carve_restated():
    """the pairs at and around every change of `waves` up to the cap, the cap itself, and the first size with waves that own no row"""
    for n in range(1, 6000):
        waves, chunk = gc.carve(n)
        assert waves == -(-n // 512) and chunk == 512 - (512 - -(-n // waves)) // 64 * 64 and waves * chunk >= n > (waves - 1) * chunk
    for n in gc.N_SIZES:
        print(n, gc.carve(n))
    want = {10: (1, 64), 63: (1, 64), 64: (1, 64), 65: (1, 128), 511: (1, 512), 512: (1, 512), 513: (2, 320), 1024: (2, 512), 1025: (3, 384),
            4608: (9, 512), 4609: (10, 512), 524288: (1024, 512), 524289: (1024, 576), 600000: (1024, 640)}
    assert {n: gc.carve(n) for n in gc.N_SIZES} == want
    for n in (524289, 600000):
        waves, chunk = gc.carve(n)
        idle = sum(1 for w in range(waves) if w * chunk >= n)
        print(f"n = {n}: waves that own no row: {idle}, of them with lo > n: {sum(1 for w in range(waves) if w * chunk > n)}")
        assert idle >= (100 if n == 524289 else 80)


@pytest.mark.parametrize("name", sorted(gc.GROUPS["N"]))
def test_sort_cases_are_all_ground(name):
    case = gc.get(name)
    res, pid = case["res"], case["pid"]
    assert np.array_equal(res["patch"], np.where(pid < 0, -1, pid))         # the rows lie where they were put
    t = res["table"]
    used = t[:, 0] > 0
    inside = pid >= 0
    print(f"{name}: {case['claim']}; patches in use {int(used.sum())}, fewest rows {int(t[used, 0].min())}, in-range rows {int(inside.sum())}, "
          f"of them ground {int((~res['nonground'][inside]).sum())}")
    assert (t[used, 0] >= 10).all() and np.isin(t[used, 12], (gr.ACCEPTED, gr.FAR)).all() and (t[used, 1] == t[used, 0]).all()
    assert not res["nonground"][inside].any() and res["nonground"][~inside].all()


def _tiles(pid):
    """the tiles of 64 rows as the scatter sees them: per binning wave from its first row on"""
    waves, chunk = gc.carve(len(pid))
    for w in range(waves):
        lo, hi = w * chunk, min((w + 1) * chunk, len(pid))
        for at in range(lo, hi, 64):
            yield w, pid[at: min(at + 64, hi)]


def test_tile_compositions():
    pid = gc.get("tile_64_patches")["pid"]
    full = [t for _, t in _tiles(pid) if len(t) == 64]
    assert len(full) == 40 and all(len(set(t)) == 64 for t in full)
    pid = gc.get("tile_one_patch")["pid"]
    kinds = [len(set(t)) for _, t in _tiles(pid)]
    assert (np.diff(pid) >= 0).all() and max(kinds) <= 2 and kinds.count(1) >= 10
    pid = gc.get("tile_two_alternating")["pid"]
    assert all(set(t[0::2]) == {7} and set(t[1::2]) == {300} for _, t in _tiles(pid))
    pid = gc.get("tile_unbinned")["pid"]
    assert gc.carve(len(pid)) == (8, 512) and (pid >= 0).sum() * 4 <= len(pid)
    empty_tiles = [(w, i) for i, (w, t) in enumerate(_tiles(pid)) if (t < 0).all()]
    empty_chunks = [w for w in range(8) if (pid[w * 512: (w + 1) * 512] < 0).all()]
    print("tile_unbinned: binned rows", int((pid >= 0).sum()), "of", len(pid), "tiles without one", empty_tiles, "chunks without one", empty_chunks)
    assert empty_chunks == [3] and any(w != 3 for w, _ in empty_tiles) and (pid == -2).any() and (pid == -1).any()
    pid = gc.get("one_patch_every_wave")["pid"]
    waves, chunk = gc.carve(len(pid))
    per_wave = [int((pid[w * chunk: (w + 1) * chunk] == 0).sum()) for w in range(waves)]
    print("one_patch_every_wave: waves", waves, "rows of patch 0 per wave", min(per_wave), "..", max(per_wave))
    assert (pid == 0).sum() == 20000 and waves >= 40 and min(per_wave) >= 1 and all((pid[w * chunk: (w + 1) * chunk] != 0).any() for w in range(waves))


# ---- L ----------------------------------------------------------------------------------------------------------------------
def _patch_changes(case, p, **wrong):
    res = case["res"]
    other = gr.segment(case["pts"], case["params"], **wrong)
    rows = res["patch"] == p
    return other, int((res["nonground"][rows] != other["nonground"][rows]).sum()), int(other["table"][p, 1] - res["table"][p, 1])


def test_ties_mixed_lows_notices_every_wrong_selection():
    case = gc.get("ties_mixed_lows")
    res, p, par, pts = case["res"], case["patch"], case["params"], case["pts"]
    z = np.sort(pts[res["patch"] == p, 2].astype(np.float64))
    a, b = z[0], z[15]
    assert (z[:15] == a).all() and (z[15:30] == b).all() and z[30] > b and a < b
    right = case["thresholds"][20]
    assert res["seeds"][p][-1] == right == (15 * a + 5 * b) / 20 + par.th_seeds
    print(f"ties_mixed_lows: a {a!r} b {b!r}, threshold {right!r}, margin of the patch {res['margin'][p]:.3e}")
    for rule in case["wrong"]:
        other, labels, count = _patch_changes(case, p, seed_rule=rule)
        thr = other["seeds"][p][-1]
        between = int(((z > min(thr, right)) & (z < max(thr, right))).sum())
        print(f"  seed_rule {rule}: threshold {thr!r} ({thr - right:+.3e}, {abs(thr - right) / par.th_seeds:.3e} of th_seeds), rows between {between}, "
              f"labels changed {labels}, ground count {count:+d}")
        assert abs(thr - right) / par.th_seeds > 1e-3 > gr.MARGIN_BAR and between >= 10
        assert labels >= 10 or count != 0
        assert labels >= 10


def test_lows_stand_at_late_places():
    case = gc.get("lows_late_places")
    res, pts = case["res"], case["pts"]
    for p, m in zip(case["patches"], case["sizes"]):
        z = pts[res["patch"] == p, 2]                                      # in row order: the places
        lowest = np.sort(np.argsort(z, kind="stable")[:20])
        print(f"lows_late_places: patch {p} of {len(z)} rows: places of its 20 lowest {lowest[0]} .. {lowest[-1]}, the lowest of all at {int(np.argmin(z))}")
        assert len(z) == m and (lowest == np.arange(m - 20, m)).all() and np.argmin(z) == m - 1 and lowest[-1] >= (m - 1) // 256 * 256
        assert res["table"][p, 1] == 20                                    # the lows alone are its ground
        for rule in case["wrong"]:
            other, labels, count = _patch_changes(case, p, seed_rule=rule)
            assert other["seeds"][p][-1] != res["seeds"][p][-1]


def test_exactly_20_and_19_after_skip():
    case = gc.get("exactly_20")
    res, par, pts = case["res"], case["params"], case["pts"]
    p20, p19 = case["patches"]
    z20, z19 = pts[res["patch"] == p20, 2].astype(np.float64), pts[res["patch"] == p19, 2].astype(np.float64)
    left = z19[~(z19 < par.skip_below)]
    print(f"exactly_20: rows {len(z20)}; 19_after_skip: rows {len(z19)}, candidates {len(left)}")
    assert len(z20) == par.num_lpr == 20 and p20 >= 32 and len(z19) == 40 and len(left) == 19 and p19 < 32
    assert res["seeds"][p20][-1] == sum(np.sort(z20)) / 20 + par.th_seeds or abs(res["seeds"][p20][-1] - (z20.mean() + par.th_seeds)) < 1e-12
    assert abs(res["seeds"][p19][-1] - (left.mean() + par.th_seeds)) < 1e-12
    other, labels, count = _patch_changes(case, p20, seed_rule=19)
    print(f"  19 seeds in exactly_20: threshold {other['seeds'][p20][-1] - res['seeds'][p20][-1]:+.3e}")
    assert abs(other["seeds"][p20][-1] - res["seeds"][p20][-1]) / par.th_seeds > 1e-3
    # a selection that did not stop when it ran dry (a 20th value from nowhere) would give another mean than these 19
    other, _, _ = _patch_changes(case, p19, seed_rule=18)
    assert abs(other["seeds"][p19][-1] - res["seeds"][p19][-1]) / par.th_seeds > 1e-3


def test_final_plane_by_and_pl_differ():
    case = gc.get("final_plane")
    other = gr.segment(case["pts"], case["params"], final_plane="pl")
    labels = int((other["nonground"] != case["res"]["nonground"]).sum())
    print("final_plane: labels that the plane fitted to the last set would change:", labels)
    assert labels >= 10 and (gr.determined(other, case["params"]) == gr.determined(case["res"], case["params"])).all()


# ---- R ----------------------------------------------------------------------------------------------------------------------
def test_list_95():
    case = gc.get("list_95")
    res = case["res"]
    assert sorted(res["rings"]) == [3]
    ring = res["rings"][3]
    t = res["table"]
    q = gr.patch_index(1, 1, 31)
    print(f"list_95: listed {len(ring['listed'])}, mu {ring['mu']:.3e}, the candidate's flatness {t[q, 10]:.3e}, outcome {int(t[q, 13])}, margin {res['margin'][q]:.3e}")
    assert len(ring["listed"]) == 95 and len(ring["own"]) == 31 and (t[:, 12] == gr.CANDIDATE).sum() == 1 and t[q, 12] == gr.CANDIDATE
    assert t[q, 13] in (gr.TGR_REVERTED, gr.TGR_REJECTED) and (t[:96, 0] >= 10).all()
    # the outcome rests on the values carried over from rings 0 to 2: by ring 3's own 31 it would be the other one
    f = t[q, 10]

    def back(values):
        v = np.float64(values)
        mu = v.mean() + 1.5 * v.std(ddof=1)
        return 1.0 / (1.0 + np.exp((f - mu) / (mu / 10.0))) > 0.5

    print("  reverted by all 95:", back(ring["listed"]), "by ring 3's own:", back(ring["own"]), "by the first 64:", back(ring["listed"][:64]))
    assert back(ring["listed"]) == (t[q, 13] == gr.TGR_REVERTED) and back(ring["listed"]) != back(ring["own"])


def test_candidates_32():
    case = gc.get("candidates_32")
    res = case["res"]
    t = res["table"][32:64]
    print("candidates_32: outcomes", [int(x) for x in t[:, 13]], "listed", len(res["rings"][2]["listed"]))
    assert (t[:, 12] == gr.CANDIDATE).all() and set(t[:, 13]) == {gr.TGR_REVERTED, gr.TGR_REJECTED} and sorted(res["rings"]) == [2]
    assert min((t[:, 13] == gr.TGR_REVERTED).sum(), (t[:, 13] == gr.TGR_REJECTED).sum()) >= 8


def test_dense_1500_and_1501():
    out = {}
    for m in (1500, 1501):
        case = gc.get(f"dense_{m}")
        t, p = case["res"]["table"], case["patch"]
        print(f"dense_{m}: ground points {int(t[p, 1])}, flatness {t[p, 10]:.3e} (th_dist^2 {case['params'].th_dist ** 2:.3e}), outcome {int(t[p, 13])}, "
              f"margin {case['res']['margin'][p]:.3e}")
        assert t[p, 1] == m == t[p, 0] and t[p, 12] == gr.CANDIDATE and t[p, 10] < case["params"].th_dist ** 2
        # the count's own margin is |m - 1500.5| / 1500 = 1 / 3000; the patch's is the smallest of all its decisions
        assert gr.MARGIN_BAR < case["res"]["margin"][p] <= 1 / 3000 + 1e-15 and gr.determined(case["res"])[p]
        out[m] = int(t[p, 13])
    assert out == {1500: gr.TGR_REJECTED, 1501: gr.TGR_REVERTED}


# ---- E ----------------------------------------------------------------------------------------------------------------------
def _sums_exactly(v):
    import math
    a = np.sort(v)
    up = down = 0.0
    for x in a:
        up += float(x)
    for x in a[::-1]:
        down += float(x)
    return math.fsum(v) == up == down


def test_exact_lattices_are_what_they_claim():
    case = gc.get("exact_lattices")
    res, pts = case["res"], case["pts"].astype(np.float64)
    t = res["table"]
    for k, p in case["patches"].items():
        rows = case["parts"][k]
        assert (res["patch"][rows] == p).all() and t[p, 0] == len(rows), k                     # each lies in its one patch
        P = pts[rows]
        exact = all(_sums_exactly(P[:, a]) for a in range(3))
        mean = P.sum(axis=0) / len(P)
        C = P - mean
        prods = all(_sums_exactly(C[:, a] * C[:, b]) for a in range(3) for b in range(a, 3))
        print(f"{k}: patch {p}, rows {len(rows)}, coordinates sum exactly {exact}, centred products sum exactly {prods}")
        assert exact and (prods or k == "copies")
        if k not in gc.E_DEGENERATE:                                        # the last plane is that of the whole patch
            assert res["covs"][p][1] == len(rows) == t[p, 1]
        if k != "flat_exact" and k != "copies":
            assert (P * 64 == np.round(P * 64)).all()
    cov = lambda k: res["covs"][case["patches"][k]][0]   # noqa: E731
    c = cov("flat_exact")
    assert c[0, 0] == c[1, 1] > 0 and (c[2] == 0).all() and c[0, 1] == 0 and (pts[case["parts"]["flat_exact"], 2] == gc.E_Z).all()
    c = cov("square_lattice")
    assert c[0, 0] == c[1, 1] > c[2, 2] > 0 and c[0, 1] == c[0, 2] == c[1, 2] == 0
    c = cov("tilt_exact")
    assert c[1, 1] == 2.0 ** -4 and c[1, 2] == c[1, 1] / 4 and c[2, 2] == c[1, 1] / 16 and c[0, 1] == c[0, 2] == 0
    theta = 0.5 * (c[2, 2] - c[1, 1]) / c[1, 2]
    assert theta == -1.875 and np.sqrt(1.0 + theta * theta) == 2.125 and c[2, 2] + (-0.25) * c[1, 2] == 0.0   # the rotation leaves exactly 0
    s = np.linalg.eigvalsh(cov("thin_strip"))[::-1]
    print(f"thin_strip: s1 / s0 {s[1] / s[0]:.3e}, (s1 - s2) / s0 {(s[1] - s[2]) / s[0]:.3e}, the restatement's gap {res['gap'][case['patches']['thin_strip']]:.3e}")
    assert s[1] / s[0] < 4e-3 and (s[1] - s[2]) / s[0] >= 3e-3 and res["gap"][case["patches"]["thin_strip"]] >= 3e-3
    r = np.hypot(*pts[case["parts"]["far_small"], 0:2].T)
    assert r.min() > 59 and r.max() < 61.5 and np.ptp(pts[case["parts"]["far_small"], 0]) < 1
    # the revert: flat_exact is the one listed value, tilt_exact the one candidate: mu = 0, rejected
    q, ring = case["patches"]["tilt_exact"], res["rings"][3]
    print("tilt_exact: code", int(t[q, 12]), "revert", int(t[q, 13]), "listed", ring["listed"], "mu", ring["mu"], "its flatness", t[q, 10])
    assert len(ring["listed"]) == 1 and abs(ring["listed"][0]) < 1e-15 and ring["mu"] == 0 and (t[q, 12], t[q, 13]) == (gr.CANDIDATE, gr.TGR_REJECTED)
    assert abs(t[q, 10]) < 1e-15 and res["nonground"][case["parts"]["tilt_exact"]].all() and not res["nonground"][case["parts"]["flat_exact"]].any()
    # the two degenerate patches: a gap of nothing
    for k in gc.E_DEGENERATE:
        p = case["patches"][k]
        print(f"{k}: gap {res['gap'][p]:.3e}")
        assert res["gap"][p] < 1e-9
    # and the restatement's neighbours are the same without them
    alone = gc.get("exact_lattices_alone")["res"]["table"]
    others = np.setdiff1d(np.arange(gr.PATCHES), case["leave_out"])
    assert (alone[list(case["leave_out"])] == 0).all() and np.array_equal(t[others][:, [0, 1, 12, 13, 14]], alone[others][:, [0, 1, 12, 13, 14]])
    assert np.array_equal(t[others], alone[others], equal_nan=True)      # (the same rows in the same order)

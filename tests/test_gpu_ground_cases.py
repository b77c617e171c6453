"""icpflow_ground_segment on its own: every input of tests/ground_cases.py (tests/test_ground_cases.py proves on the CPU what each
one is) through the raw C ABI (tests/ground_device.py: the case's own parameters, an exactly sized workspace filled with 0xFF,
guards around it and around both outputs) against the fp64 restatement at the same parameters, with the assertions of
tests/test_gpu_ground.py::compare and no row and no patch left out -- but the two degenerate patches that group E names.
Every case runs twice on one workspace and once on a second stream, bit-identical.  Every figure is printed before it is
asserted.

The singular values of group E.  The reference is the eigenvalues, by mpmath at 40 digits, of the covariance the restatement
forms from the same set -- on these lattices the moments are exact, so it is the kernel's covariance bit for bit.  The bound
is C * 2^-53 * s0 with C = 512, derived, not measured: cyclic Jacobi replaces A by R^T A R, and what one rotation computes is
the exact transform of A + E.  E has the four entries the rotation recomputes (a_pp, a_qq, a_rp, a_rq, mirrored); each is
a short expression in t, c, s and tau -- themselves 4 to 6 roundings from their inputs -- and comes out within 8 * 2^-53 * |A|:
|E|_2 <= |E|_F <= sqrt(6) * 8 * 2^-53 |A| < 20 * 2^-53 |A|.  A 3 x 3 converges quadratically: 6 sweeps of 3 rotations are more than
it takes (a sweep beyond the fourth zeroes what is below 2^-53 outright), 18 * 20 = 360, and an eigenvalue moves by no more
than |E|_2 (Weyl).  512 leaves room for the final division by m - 1; it is 5.7e-14 relative.  (Measured, for orientation only: at most
1.4 of these units on the five lattices, COVERAGE.md.)
A normal is held to that bound divided by the gap (s1 - s2) / s0 (Davis-Kahan), against mpmath's eigenvector."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_cases as gc            # noqa: E402
import ground_device as gd           # noqa: E402
import ground_restatement as gr      # noqa: E402

pytestmark = pytest.mark.gpu
C_JACOBI = 512.0
U = 2.0 ** -53
WORST = dict(plane=(0.0, ""), sv=(0.0, ""))


def check(name, **form):
    """the case through the C ABI: compared with the restatement, then again on the same workspace and on a second stream"""
    case = gc.get(name)
    pts, par, res = case["pts"], case["params"], case["res"]
    bufs = gd.Buffers(len(pts), par)
    first = gd.run(pts, par, buffers=bufs, **form)
    kept, det, worst = gd.compare(name, res, *first, params=par, leave_out=case.get("leave_out", ()))
    if worst > WORST["plane"][0]:
        WORST["plane"] = (worst, name)
    left = sum(int((res["patch"] == p).sum()) for p in case.get("leave_out", ()))
    assert kept == len(pts) - left                                          # no row left out
    again = gd.run(pts, par, buffers=bufs, **form)                          # the workspace as the first call left it
    side = gd.run(pts, par, stream=torch.cuda.Stream(gd.DEV), **form)
    assert gd.same_bits(first, again) and gd.same_bits(first, side), name
    return first


@pytest.mark.parametrize("name", sorted(gc.GROUPS["P"]))
def test_parameters(name):
    check(name)


@pytest.mark.parametrize("name", sorted(gc.GROUPS["L"]) + sorted(gc.GROUPS["R"]))
def test_seeds_and_revert(name):
    labels, table = check(name)
    case = gc.get(name)
    if name.startswith("dense_"):
        assert table[case["patch"], 1] == int(name[6:]) and table[case["patch"], 13] == (gr.TGR_REVERTED if name == "dense_1501" else gr.TGR_REJECTED)
    if name == "list_95":
        assert table[gr.patch_index(1, 1, 31), 13] == gr.TGR_REVERTED
    if name == "candidates_32":
        assert set(table[32:64, 13]) == {gr.TGR_REVERTED, gr.TGR_REJECTED}


@pytest.mark.parametrize("name", sorted(gc.GROUPS["N"]))
def test_counting_sort(name):
    labels, table = check(name)
    pid = gc.get(name)["pid"]
    assert not labels[pid >= 0].any() and labels[pid < 0].all()             # all ground: a row lost or misfiled shows
    assert np.array_equal(table[:, 0], np.bincount(pid[pid >= 0], minlength=gr.PATCHES)) and (table[:, 1] == table[:, 0]).all()


def test_strides_offsets_and_forms():
    name = "strides_mixed"
    want = check(name)
    pts, par = gc.get(name)["pts"], gc.get(name)["params"]
    for stride in (3, 4, 5, 16):
        for fill in (np.nan, 1e30):
            for offset in ((0, 4, 8) if stride in (3, 5) else (0,)):
                got = gd.run(pts, par, stride=stride, offset=offset, fill=fill)
                same = gd.same_bits(want, got)
                print(f"stride {stride}, other columns {fill}, base + {offset}: same bits {same}")
                assert same, (stride, fill, offset)
    for stride, offset in ((3, 0), (5, 4)):                                 # without a table: the same labels, no table byte written
        labels, none = gd.run(pts, par, stride=stride, offset=offset, with_table=False)
        assert none is None and np.array_equal(labels, want[0])
    labels, none = gd.run(pts[:0], par)                                     # n == 0: status 0, nothing written
    assert labels.shape == (0,) and none is None


# ---- E ----------------------------------------------------------------------------------------------------------------------
def _eig(cov):
    """eigenvalues descending and the eigenvector of the smallest (z >= 0) by mpmath at 40 digits"""
    import mpmath
    with mpmath.workdps(40):
        E, Q = mpmath.eigsy(mpmath.matrix(cov.tolist()))
        order = sorted(range(3), key=lambda k: E[k], reverse=True)
        vals = [E[k] for k in order]
        v = [Q[r, order[2]] for r in range(3)]
        if v[2] < 0:
            v = [-x for x in v]
        return vals, v


def test_plane_solve_on_exact_lattices():
    labels, table = check("exact_lattices")
    case = gc.get("exact_lattices")
    res, pts, at = case["res"], case["pts"].astype(np.float64), case["patches"]
    import mpmath
    for k in ("flat_exact", "tilt_exact", "square_lattice", "thin_strip", "far_small"):
        p = at[k]
        cov, m = res["covs"][p]
        rows = np.flatnonzero(res["patch"] == p)
        assert m == len(rows) == table[p, 1]                                 # the last set is the whole patch
        vals, v = _eig(cov)
        s0 = float(vals[0])
        gap = float((vals[1] - vals[2]) / vals[0])
        with mpmath.workdps(40):
            err = max(abs(mpmath.mpf(float(table[p, 8 + i])) - abs(vals[i])) for i in range(3))
            nerr = max(abs(mpmath.mpf(float(table[p, 5 + i])) - v[i]) for i in range(3)) if gap > 0 else None
        units = float(err) / (U * s0)
        print(f"{k}: s = {table[p, 8:11]}, |s - eigenvalue| {units:.2f} x 2^-53 s0 (bound {C_JACOBI:.0f}), gap {gap:.3e}" +
              (f", |normal - eigenvector| {float(nerr):.3e} (bound {C_JACOBI * U / gap:.3e})" if k != "square_lattice" else ""))
        if units > WORST["sv"][0]:
            WORST["sv"] = (units, k)
        assert units <= C_JACOBI
        if k != "square_lattice":                                            # (s0 == s1 there; the normal is the third vector and has its gap)
            assert float(nerr) <= C_JACOBI * U / gap
        mean = np.array([math.fsum(pts[rows, a]) / m for a in range(3)])
        assert np.array_equal(table[p, 2:5], mean), k                        # the sums are exact: one division each
    z = float(gc.E_Z)
    f = table[at["flat_exact"]]
    print("flat_exact:", f[5:12])
    assert f[10] == 0.0 and np.array_equal(f[5:8], [0.0, 0.0, 1.0]) and f[11] == -z and f[12] == gr.ACCEPTED
    t = table[at["tilt_exact"]]
    print("tilt_exact:", t[5:14])
    assert t[10] == 0.0 and (t[12], t[13]) == (gr.CANDIDATE, gr.TGR_REJECTED)      # flatness 0 against a list of one 0: 0 / 0, rejected
    assert labels[case["parts"]["tilt_exact"]].all() and not labels[case["parts"]["flat_exact"]].any()
    q = table[at["square_lattice"]]
    assert q[8] == q[9] > q[10] > 0 and np.array_equal(q[5:8], [0.0, 0.0, 1.0])
    # the two named degenerate patches: the count, every entry finite (a NaN plane is a single point's alone), the same bits again
    for k in gc.E_DEGENERATE:
        row = table[at[k]]
        print(f"{k}: {row}")
        assert row[0] == len(case["parts"][k]) and np.isfinite(row).all() and 0 <= row[1] <= row[0] and row[12] in range(1, 6)
    # ... and their neighbours in the same call come out as without them, bit for bit
    alone_labels, alone = check("exact_lattices_alone")
    others = np.setdiff1d(np.arange(gr.PATCHES), case["leave_out"])
    assert np.array_equal(table[others].view(np.uint64), alone[others].view(np.uint64))
    keep = ~np.isin(res["patch"], case["leave_out"])
    assert np.array_equal(labels[keep], alone_labels)


def test_zz_report():
    """the largest figures of this module, for COVERAGE.md"""
    print(f"largest |plane - restatement| {WORST['plane'][0]:.3e} ({WORST['plane'][1]}); largest singular-value error "
          f"{WORST['sv'][0]:.2f} x 2^-53 s0 ({WORST['sv'][1]})")
    assert WORST["plane"][0] <= gd.TOL and WORST["sv"][0] <= C_JACOBI

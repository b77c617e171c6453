"""CPU only: tests/peak_restatement.py against the reference's formula, evaluated by torch (max_pool3d(x, ks, 1, (ks - 1) // 2) == x,
utils_hist.py: topk_nms), on every volume of tests/peak_cases.py whose values fit a float32 -- and every case asserted to be what
its name says: the window-face pairs suppressed or not, the survivors' counts, and on the permutation volumes that each face of the
window, moved by one step, changes the expected output (so a kernel with that window cannot pass tests/test_gpu_peaks.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_cases as pc                  # noqa: E402
import peak_restatement as pr            # noqa: E402


def every_case():
    out = [pc.hand()]
    out += [c for s, ks in pc.FACE_SHAPES for c in pc.faces_parts(s, ks)]
    out += [pc.permutation(s, ks, B) for s, ks, B in pc.PERMUTATION_SHAPES]
    out += [pc.lines(s) for s in pc.LINE_SHAPES]
    out += [pc.survivors_ks1(n) for n in pc.LIST_COUNTS] + [pc.survivors_ks11(n) for n in pc.LIST_COUNTS]
    out += [pc.seam(s, ks, kind) for s in pc.SEAM_SHAPES for ks in (11, 3) for kind in ("permutation", "plateau")]
    out += [pc.permutation(s, ks, 3) for s, ks in pc.U32_SHAPES]
    out += [pc.large_votes(1), pc.large_votes(3)]
    return out


CASES = every_case()


def reference(vol, k, ks):
    """utils_hist.py: topk_nms with the tie rule of icpflow_hist_peaks -> (surviving mask [B, L], votes float32 [B, k], idx [B, k])"""
    x = torch.from_numpy(vol.astype(np.float32))[:, None]
    keep = F.max_pool3d(x, kernel_size=ks, stride=1, padding=(ks - 1) // 2) == x
    sv = (x * keep).reshape(len(vol), -1)
    votes, idx = torch.sort(sv, dim=1, descending=True, stable=True)      # stable: equal votes stay in ascending flat index
    return keep.reshape(len(vol), -1).numpy(), votes[:, :k].numpy(), idx[:, :k].numpy()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_max_pool3d(case):
    vol = case["vol"]
    if int(vol.max()) >= 1 << 24:
        assert case["name"].startswith("large votes")                     # (the only volumes a float32 cannot hold)
        return
    for k in sorted({1, 5, case["k"]}):
        keep, votes, idx = reference(vol, k, case["ks"])
        r = pr.radii(case["ks"])
        mine = vol.reshape(len(vol), -1) == pr.window_max(vol, r, r).reshape(len(vol), -1)
        assert np.array_equal(mine, keep), case["name"]
        v, i = pr.peaks(vol, k, case["ks"])
        assert v.dtype == np.float32 and i.dtype == np.int64
        assert np.array_equal(v, votes), case["name"]
        assert np.array_equal(i, idx), case["name"]


def test_restatement_by_hand():
    """1 x 5 x 1 at window 3, and separate radii: lower 1 / upper 0 looks down only."""
    h = np.array([2, 0, 2, 1, 0], np.int64).reshape(1, 1, 5, 1)
    assert pr.window_max(h, (1, 1, 1), (1, 1, 1)).ravel().tolist() == [2, 2, 2, 2, 1]
    assert pr.window_max(h, (0, 1, 0), (0, 0, 0)).ravel().tolist() == [2, 2, 2, 2, 1]
    assert pr.window_max(h, (0, 0, 0), (0, 1, 0)).ravel().tolist() == [2, 2, 2, 1, 0]
    assert pr.window_max(h, (0, 2, 0), (0, 0, 0)).ravel().tolist() == [2, 2, 2, 2, 2]
    v, i = pr.peaks(h, 4, 3)
    assert i.tolist() == [[0, 2, 1, 3]] and v.tolist() == [[2, 2, 0, 0]]
    big = np.array([2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1, 2 ** 31], np.int64).reshape(1, 4, 1, 1)
    v, i = pr.peaks(big, 4, 1)
    assert i.tolist() == [[2, 3, 1, 0]] and v.tolist() == [[2.0 ** 32, 2.0 ** 31, 2.0 ** 24, 2.0 ** 24]]
    c = pr.candidates(np.array([[7, 0]]), (2, 2, 3), ([10, 11], [20, 21], [30, 31, 32]), 0.25)
    assert c.tolist() == [[[11.25, 20.25, 31.25], [10.25, 20.25, 30.25], [0, 0, 0]]]


def test_the_hand_case():
    c = pc.hand()
    v, i = pr.peaks(c["vol"], c["k"], c["ks"])
    assert v.tolist() == c["want_votes"] and i.tolist() == c["want_idx"]
    assert (v[0].tolist(), i[0].tolist()) == ([9, 5], [38, 36])           # the table of the issue: max_pool3d's answer
    lo, hi = pr.parent_z_radii(c["shape"], c["ks"])                       # ... and what the whole-column shortcut made of it
    v, i = pr.peaks(c["vol"], c["k"], lo=lo, hi=hi)
    assert (v[0].tolist(), i[0].tolist()) == ([9, 0], [38, 0])


@pytest.mark.parametrize("shape,ks", pc.FACE_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-ks{ks}" for s, ks in pc.FACE_SHAPES])
def test_window_faces_are_what_they_say(shape, ks):
    c = pc.faces(shape, ks)
    r = (ks - 1) // 2
    sv = pr.surviving(c["vol"], ks)
    v, i = pr.peaks(c["vol"], 8, ks)
    seen = set()
    for p, (axis, direction, d, big, small, survives) in enumerate(c["pairs"]):
        vol = c["vol"][p].ravel()
        assert np.count_nonzero(vol) == 2 and vol[big] > vol[small] > 0                    # distinct values, background 0
        assert sv[p, big] == vol[big] and sv[p, small] == (vol[small] if survives else 0), (p, axis, direction, d)
        assert (v[p] > 0).sum() == (2 if survives else 1) and (v[p] == 0).sum() >= 6         # survivors and the zero fill
        if axis < 3:
            assert survives == (d == r + 1) and (d in (r, r + 1) or d == shape[axis] - 1 < r)
            lo = min(np.unravel_index(big, shape)[axis], np.unravel_index(small, shape)[axis])
            seen.add((axis, direction, d, "first" if lo == 0 else "last" if lo + d == shape[axis] - 1 else "inside"))
    for axis in range(3):
        for d in (r, r + 1):
            if d <= shape[axis] - 1:
                for direction in (+1, -1):
                    assert (axis, direction, d, "first") in seen and ((axis, direction, d, "last") in seen or d == shape[axis] - 1)
    assert c["z_branch"] == pc.z_branch(shape, ks)


def test_window_faces_reach_every_z_branch():
    lds = {(ks, pc.z_branch(s, ks), "in the suspected range" if pr.parent_z_radii(s, ks) else "") for s, ks in pc.FACE_SHAPES}
    for ks in (11, 7, 5, 3):
        r = (ks - 1) // 2
        assert (ks, "general loop", "in the suspected range") in lds and (ks, "general loop", "") in lds
        assert (ks, "whole column", "") in lds or (ks, "column of 3", "") in lds
        lz = {s[2] for s, k_ in pc.FACE_SHAPES if k_ == ks and pc.form(s) == "lds"}
        assert {r + 2, 2 * r + 1, 2 * r + 2} <= lz and (r + 1 in lz or ks == 5)
    assert (11, "column of 3", "") in lds and (11, "whole column", "") in lds
    assert any(pc.form(s) == "global" for s, _ in pc.FACE_SHAPES)


def _one_step_windows(r):
    """axis, name, (lo, hi): the four windows that are wrong by one step on one face of one axis."""
    for axis in range(3):
        for name, dlo, dhi in (("lower - 1", -1, 0), ("lower + 1", +1, 0), ("upper - 1", 0, -1), ("upper + 1", 0, +1)):
            lo, hi = [r, r, r], [r, r, r]
            lo[axis] += dlo
            hi[axis] += dhi
            yield axis, name, (tuple(lo), tuple(hi))


def _changed(case, lo, hi):
    wv, wi = pr.peaks(case["vol"], case["k"], case["ks"])
    v, i = pr.peaks(case["vol"], case["k"], lo=lo, hi=hi)
    return int(((v != wv) | (i != wi)).any(axis=1).sum())


PERM_IDS = [f"{s[0]}x{s[1]}x{s[2]}-ks{ks}" for s, ks, _ in pc.PERMUTATION_SHAPES]


@pytest.mark.parametrize("shape,ks,B", pc.PERMUTATION_SHAPES, ids=PERM_IDS)
def test_permutation_volumes_notice_every_window_that_is_one_step_wrong(shape, ks, B):
    c = pc.permutation(shape, ks, B)
    r = (ks - 1) // 2
    assert len(c["vol"]) == B and all(sorted(v.ravel().tolist()) == list(range(1, v.size + 1)) for v in c["vol"][:2])
    counts = {}
    for axis, name, (lo, hi) in _one_step_windows(r):
        if shape[axis] >= r + 2:
            counts[(axis, name)] = _changed(c, lo, hi)
    print(c["name"], "pairs changed by each one-step window:", counts)
    assert counts and all(n >= 1 for n in counts.values()), counts
    z = pr.parent_z_radii(shape, ks)
    if z is not None:                                                     # inside the range of the whole-column shortcut as it was
        n = _changed(c, *z)
        print(c["name"], "pairs changed by the whole-column z window:", n)
        assert n >= 1


def test_permutation_volumes_cover_every_axis_in_every_form():
    covered = set()
    for shape, ks, _ in pc.PERMUTATION_SHAPES:
        r = (ks - 1) // 2
        kind = "global" if pc.form(shape) == "global" else "lds ks11" if ks == 11 else "lds other"
        covered |= {(kind, axis) for axis in range(3) if shape[axis] >= r + 2}
    assert covered == {(kind, axis) for kind in ("global", "lds ks11", "lds other") for axis in range(3)}
    outside = [(s, ks) for s, ks, _ in pc.PERMUTATION_SHAPES if pc.form(s) == "lds" and pr.parent_z_radii(s, ks) is None]
    assert ((7, 6, 8), 5) in outside and ((23, 25, 3), 11) in outside


def test_line_shapes_straddle_the_segment_seams():
    assert {s[0] for s in pc.LINE_SHAPES[:8]} == {s[1] for s in pc.LINE_SHAPES[:8]} == {10, 11, 12, 21, 22, 23, 33, 34}
    assert all(pc.form(s) == "lds" for s in pc.LINE_SHAPES)
    assert pc.line_items((12, 34, 31)) == (1488, 2108) and min(pc.lines((12, 34, 31))["items"]) > 1024
    for s in pc.LINE_SHAPES:                                              # permutation values, and the window matters in them
        c = pc.lines(s)
        assert sorted(c["vol"][0].ravel().tolist()) == list(range(1, c["vol"][0].size + 1))
        for axis in (0, 1):
            if s[axis] >= 7:
                assert any(_changed(c, lo, hi) for a, _, (lo, hi) in _one_step_windows(5) if a == axis), (s, axis)


@pytest.mark.parametrize("n", pc.LIST_COUNTS)
def test_survivor_counts_are_exact(n):
    for c in (pc.survivors_ks1(n), pc.survivors_ks11(n)):
        assert pr.count_positive(c["vol"], c["ks"]).tolist() == [n, n, n], c["name"]
        v, i = pr.peaks(c["vol"], 8, c["ks"])
        flat = c["vol"].reshape(3, -1)
        positive = [np.flatnonzero(pr.surviving(c["vol"], c["ks"])[b]) for b in range(3)]
        if 1 <= n <= 7:                                                   # the fill steps over the survivors in the first bins
            assert all(p.tolist() == list(range(n)) for p in positive)
            assert all(sorted(i[b, n:].tolist()) == list(range(n, 8)) and not v[b, n:].any() for b in range(3))
            if c["ks"] == 11:                                             # ... and hands out a suppressed positive bin as a zero vote
                assert (flat[:, n] > 0).all() and (i[:, n] == n).all()
        elif n >= 8 and n < pc.LIST_L:                                    # the eight largest votes sit at the highest flat indices
            assert sorted(i[0].tolist()) == positive[0][-8:].tolist() and (v[0] >= 10).all()
        elif n == 0:
            assert not v.any() and i.tolist() == [list(range(8))] * 3
    assert pc.LIST == 512 and {511, 512, 513} <= set(pc.LIST_COUNTS)


def test_seam_shapes_are_the_last_lds_volume_and_the_first_global_one():
    assert [int(np.prod(s)) for s in pc.SEAM_SHAPES] == [12800, 12801] and pc.LDS_BINS == 12800
    assert [pc.form(s) for s in pc.SEAM_SHAPES] == ["lds", "global"]
    assert 3 * 4 * 12800 == 150 * 1024
    largest = max(c["vol"].size for c in CASES)
    assert largest == 16 * 13020                                          # the largest batch the GPU file uploads


def test_large_votes_are_ordered_as_integers():
    for ks in (1, 3):
        c = pc.large_votes(ks)
        assert c["shape"][2] in range(7, 12) and len(set(c["shape"])) == 3
        assert all(set(pc.LARGE) <= set(v.ravel().tolist()) for v in c["vol"])
        v, i = pr.peaks(c["vol"], 8, ks)
        got = np.take_along_axis(c["vol"].reshape(3, -1), i, axis=1)
        assert (np.diff(got, axis=1) < 0).all()                           # strictly descending as integers ...
        assert np.array_equal(v, got.astype(np.float32))
        assert ks != 1 or (np.diff(v, axis=1) == 0).any()                 # ... with equal float32 votes among them
    top = np.take_along_axis(pc.large_votes(1)["vol"].reshape(3, -1), pr.peaks(pc.large_votes(1)["vol"], 8, 1)[1], axis=1)
    assert top[0].tolist() == sorted(pc.LARGE, reverse=True)[:8]
    for s, ks in pc.U32_SHAPES:
        assert len(set(s)) == 3
    assert any(7 <= s[2] <= 11 for s, _ in pc.U32_SHAPES)
    e = pc.edges((4, 5, 6))
    assert [x.tolist()[:2] for x in e] == [[1000, 1001], [2000, 2001], [3000, 3001]] and [len(x) for x in e] == [4, 5, 6]

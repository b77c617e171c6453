"""The peak search on its own (csrc/hist.hip hist_peaks_kernel, row a-2): icpflow_hist_peaks on float bins and
icpflow_selftest_peaks_u32 -- the instantiation the pipeline runs, uint32 counters and the fused candidate decode -- against
tests/peak_restatement.py on the volumes of tests/peak_cases.py: every face of the window on every pass form, the seam of the survivors'
list, the zero-vote fill, the seam between LDS and global scratch, the decode.  Every call runs on a workspace of exactly the documented
size between guards, with poisoned outputs (tests/peak_device.py), once more on the same stream and on a second one; everything is
array_equal.  What each case is, is asserted without a GPU in tests/test_peak_restatement.py.

Run on the MI355X box:  python -m pytest tests/test_gpu_peaks.py -m gpu -q
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import peak_cases as pc                  # noqa: E402
import peak_device as pd                 # noqa: E402
import peak_restatement as pr            # noqa: E402


def _id(shape, ks):
    return f"{shape[0]}x{shape[1]}x{shape[2]}-ks{ks}"


def test_the_hand_case():
    """5 x 5 x 3 at kernel_size 3: a 5 at z = 0 and a 9 at z = 2 of one column are outside each other's window."""
    c = pc.hand()
    for entry in ("f32", "u32"):
        got = pd.run(c["vol"], c["k"], c["ks"], entry)
        print(entry, "votes", got["votes"].tolist(), "idx", got["idx"].tolist())
        assert got["idx"].tolist() == c["want_idx"] and got["votes"].tolist() == c["want_votes"], entry
    pd.check(c)


@pytest.mark.parametrize("shape,ks", pc.FACE_SHAPES, ids=[_id(s, ks) for s, ks in pc.FACE_SHAPES])
def test_window_faces(shape, ks):
    """Two distinct values `radius` apart (the smaller is suppressed) and `radius + 1` apart (it survives), along every axis in
    both directions, at the first rows, the last rows and inside; the box's corner."""
    for c in pc.faces_parts(shape, ks):
        wv, wi = pd.check(c)
        for p, (axis, direction, d, big, small, survives) in enumerate(c["pairs"]):
            assert wi[p, 0] == big and (wi[p, 1] == small and wv[p, 1] > 0) == survives     # (the restatement's own answer, spelled out)


@pytest.mark.parametrize("shape,ks,B", pc.PERMUTATION_SHAPES, ids=[_id(s, ks) for s, ks, _ in pc.PERMUTATION_SHAPES])
def test_permutation_volumes(shape, ks, B):
    """Permutations of 1 .. L: each face of the window, moved by one step, changes the answer of some volume of the batch."""
    pd.check(pc.permutation(shape, ks, B))


@pytest.mark.parametrize("shape", pc.LINE_SHAPES, ids=[_id(s, 11) for s in pc.LINE_SHAPES])
def test_line_segments(shape):
    """Running maxima along lines: Ly and Lx on both sides of the seams of the 11-bin segments; more items than threads."""
    pd.check(pc.lines(shape))


@pytest.mark.parametrize("n", pc.LIST_COUNTS)
@pytest.mark.parametrize("ks", [1, 11])
def test_survivors_list(ks, n):
    """Exactly n positive survivors, around k and around the list's 512 places, the largest at the highest flat indices."""
    c = pc.survivors_ks1(n) if ks == 1 else pc.survivors_ks11(n)
    for k in (1, 5, 8):
        pd.check(c, k=k)


@pytest.mark.parametrize("ks", [11, 3])
@pytest.mark.parametrize("shape", pc.SEAM_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in pc.SEAM_SHAPES])
def test_lds_global_seam(shape, ks):
    """12800 bins: the largest volume in LDS; 12801: the first in global scratch."""
    for kind in ("permutation", "plateau"):
        pd.check(pc.seam(shape, ks, kind))


@pytest.mark.parametrize("ks", [1, 3])
def test_u32_votes_beyond_float32_are_ordered_as_integers(ks):
    """2^24 + 1, 2^31, 2^32 - 1 ...: compared as integers, returned as float32(vote)."""
    c = pc.large_votes(ks)
    wv, wi = pd.check(c)
    got = np.take_along_axis(c["vol"].reshape(len(wi), -1), wi, axis=1)
    assert np.array_equal(wv, got.astype(np.float32))


@pytest.mark.parametrize("shape,ks", pc.U32_SHAPES, ids=[_id(s, ks) for s, ks in pc.U32_SHAPES])
def test_u32_decode(shape, ks):
    """Lx != Ly != Lz, edges that differ per axis and per bin: candidates [B, k + 1, 3] are float32(e[i] + shift) bit for bit, the zero
    translation last; without d_cand the same votes and indices."""
    c = pc.permutation(shape, ks, 3)
    for k in (1, 5, 8):
        wv, wi = pd.check(c, k=k)
        plain = pd.run(c["vol"], k, ks, "u32", decode=False)
        assert plain["cand"] is None and np.array_equal(plain["idx"], wi) and np.array_equal(plain["votes"], wv)
        wc = pr.candidates(wi, shape, pc.edges(shape), pc.SHIFT)
        assert wc.shape == (3, k + 1, 3) and (wc[:, :-1, 0] >= 1000).all() and (wc[:, :-1, 0] < 2000).all()
        assert (wc[:, :-1, 1] >= 2000).all() and (wc[:, :-1, 2] >= 3000).all() and not wc[:, -1].any()

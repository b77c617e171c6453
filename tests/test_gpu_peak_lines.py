"""The peak search (hist_peaks_kernel through utils_hist.topk_nms) against a NumPy restatement, exactly: the window maximum
along lines, the survivors' list and its fall-back, the zero-vote fill.  The search is a pure function of an integer volume
(maxima and comparisons), so votes and indices must be EQUAL, whatever the shape, the window or k.

Run on the MI355X box:  python -m pytest tests/test_gpu_peak_lines.py -m gpu -q
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import utils_hist  # noqa: E402

DEV = torch.device("cuda:0")
B = 3     # the first and the last pair of a batch are both covered


def box_max(h, radius):
    """Maximum over the clamped box |dx|, |dy|, |dz| <= radius of a [B, Lx, Ly, Lz] volume (separable)."""
    out = h.copy()
    for axis in (1, 2, 3):
        n = out.shape[axis]
        acc = out.copy()
        for d in range(1, min(radius, n - 1) + 1):
            lo = [slice(None)] * 4
            hi = [slice(None)] * 4
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            acc[tuple(lo)] = np.maximum(acc[tuple(lo)], out[tuple(hi)])     # the neighbour d above
            acc[tuple(hi)] = np.maximum(acc[tuple(hi)], out[tuple(lo)])     # ... and d below
        out = acc
    return out


def topk_nms_numpy(h, k, kernel_size):
    """utils_hist.topk_nms restated: surviving vote = h where h equals its window's maximum, else 0; every bin takes part;
    order by (vote descending, flat index ascending) -- zero votes therefore fill up from flat index 0."""
    h = h.astype(np.int64)
    sv = np.where(h == box_max(h, (kernel_size - 1) // 2), h, 0).reshape(len(h), -1)
    votes = np.empty((len(h), k), np.float32)
    idx = np.empty((len(h), k), np.int64)
    for b in range(len(h)):
        order = np.lexsort((np.arange(sv.shape[1]), -sv[b]))[:k]
        votes[b], idx[b] = sv[b][order], order
    return votes, idx


@functools.lru_cache(maxsize=None)
def volumes(shape, radius):
    """name -> [B, Lx, Ly, Lz] int64 volume of small non-negative integers, for one shape."""
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + shape[2])
    full = (B,) + shape
    L = int(np.prod(shape))
    out = {}
    out["sparse ties"] = rng.integers(0, 4, size=full) * (rng.random(full) < 0.05)
    out["dense"] = rng.integers(0, 1001, size=full)
    out["all zero"] = np.zeros(full, np.int64)
    corners = [(x, y, z) for x in (0, shape[0] - 1) for y in (0, shape[1] - 1) for z in (0, shape[2] - 1)]
    for g in range(3):                                             # eight corners in turn, three per batch
        v = np.zeros(full, np.int64)
        for b in range(B):
            v[(b,) + corners[(3 * g + b) % 8]] = 7 + b
        out[f"corners {g}"] = v
    out["constant"] = np.full(full, 3, np.int64)                  # every bin survives: beyond any list of survivors
    # fewer than k positive survivors: the zero-vote fill has to step over a survivor at flat index 1 and takes the
    # suppressed (positive, not surviving) bin at flat index 2
    v = np.zeros((B, L), np.int64)
    v[:, 1], v[:, min(2, L - 1)] = 5, 1
    v[1, L - 1] = 9
    v[2, L // 2] = 5
    out["few survivors"] = v.reshape(full)
    # two equal maxima exactly radius and radius + 1 apart along each axis (pair b: axis b), where the axis is long enough
    for d in (radius, radius + 1):
        v = np.zeros(full, np.int64)
        for axis in range(3):
            p = [shape[0] // 3, shape[1] // 3, shape[2] // 3]
            p[axis] = 0 if shape[axis] <= d + 1 else min(1, shape[axis] - d - 1)
            v[(axis,) + tuple(p)] = 4
            if d > 0 and shape[axis] > d:
                p[axis] += d
                v[(axis,) + tuple(p)] = 4
            v[axis] += (rng.random(shape) < 0.02) * (v[axis] == 0)          # (and a few single votes around them)
        out[f"window edge {d}"] = v
    return out


CASES = [((41, 41, 3), 11, 5),                                    # the headline path
         ((3, 41, 3), 11, 5), ((41, 3, 3), 11, 5),                # a line shorter than the window
         ((12, 23, 3), 11, 5), ((11, 11, 1), 11, 5), ((5, 7, 4), 11, 5), ((64, 3, 2), 11, 5),
         ((41, 41, 3), 11, 1), ((41, 41, 3), 11, 8),
         ((41, 41, 3), 1, 5), ((41, 41, 3), 3, 5), ((41, 41, 3), 7, 5),     # radius 0 and the general-radius loop
         ((120, 120, 3), 11, 5)]                                  # volumes in global scratch, the same entry


@pytest.mark.parametrize("shape,kernel_size,k", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-ks{ks}-k{k}" for s, ks, k in CASES])
def test_peaks_equal_the_numpy_restatement(shape, kernel_size, k):
    for name, vol in volumes(shape, (kernel_size - 1) // 2).items():
        wv, wi = topk_nms_numpy(vol, k, kernel_size)
        v, i = utils_hist.topk_nms(torch.from_numpy(vol.astype(np.float32)).to(DEV), k=k, kernel_size=kernel_size)
        v, i = v.cpu().numpy(), i.cpu().numpy()
        assert np.array_equal(i, wi), (name, i, wi)
        assert np.array_equal(v, wv), (name, v, wv)


def test_the_restatement_itself():
    """The NumPy side on a volume small enough to check by hand: 1 x 5 x 1, window 3."""
    h = np.array([2, 0, 2, 1, 0], np.int64).reshape(1, 1, 5, 1)
    assert box_max(h, 1).ravel().tolist() == [2, 2, 2, 2, 1]
    v, i = topk_nms_numpy(h, 4, 3)
    assert i.tolist() == [[0, 2, 1, 3]] and v.tolist() == [[2, 2, 0, 0]]

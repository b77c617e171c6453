"""The peak search (icpflow_hist_peaks / hist_peaks_kernel, utils_hist.topk_nms of the reference) restated in NumPy, integers only.
Not a test module.

    surviving vote = h where h equals the maximum of h over the clamped box  -lo <= d <= hi  per axis, 0 elsewhere
    (the operation itself: lo = hi = (kernel_size - 1) // 2 on all three axes);
    every bin takes part; order (vote descending, flat index ascending); votes returned as float32(vote).

The lower and the upper radius of every axis are separate arguments, so that a test can state a window that is wrong by one
step on one face and ask whether a volume would notice (tests/test_peak_restatement.py)."""
import numpy as np


def radii(kernel_size):
    r = (int(kernel_size) - 1) // 2
    return (r, r, r)


def window_max(h, lo, hi):
    """h int64 [B, Lx, Ly, Lz] -> the maximum over x - lo[0] <= x' <= x + hi[0], ... (positions outside the volume do not exist).
    One axis after the other: the maximum over a box is the maximum over its rows of the maxima over its columns."""
    out = np.asarray(h, np.int64)
    assert out.ndim == 4 and all(int(r) >= 0 for r in tuple(lo) + tuple(hi))
    for axis in (3, 2, 1):
        n = out.shape[axis]
        acc = out.copy()
        for sign, reach in ((+1, int(hi[axis - 1])), (-1, int(lo[axis - 1]))):
            for d in range(1, min(reach, n - 1) + 1):
                here, there = [slice(None)] * 4, [slice(None)] * 4
                # sign +1: position q looks at q + d (q = 0 .. n - d - 1); sign -1: q looks at q - d (q = d .. n - 1)
                here[axis], there[axis] = (slice(0, n - d), slice(d, n)) if sign > 0 else (slice(d, n), slice(0, n - d))
                np.maximum(acc[tuple(here)], out[tuple(there)], out=acc[tuple(here)])
        out = acc
    return out


def surviving(h, kernel_size=None, lo=None, hi=None):
    """-> int64 [B, L]: the surviving votes, flattened per volume."""
    h = np.asarray(h, np.int64)
    assert (h >= 0).all() and (h < 2 ** 32).all(), "bins are vote counts: uint32"
    if kernel_size is not None:
        lo = hi = radii(kernel_size)
    return np.where(h == window_max(h, lo, hi), h, 0).reshape(len(h), -1)


def count_positive(h, kernel_size):
    """-> int64 [B]: bins with a positive surviving vote (what the kernel's list holds)."""
    return (surviving(h, kernel_size) > 0).sum(axis=1)


def peaks(h, k, kernel_size=None, lo=None, hi=None):
    """-> (votes float32 [B, k], idx int64 [B, k])."""
    sv = surviving(h, kernel_size, lo, hi)
    assert 1 <= k <= sv.shape[1]
    # a stable sort of the negated votes: equal votes stay in ascending flat index
    idx = np.argsort(-sv, axis=1, kind="stable")[:, :k].astype(np.int64)
    votes = np.take_along_axis(sv, idx, axis=1)
    return votes.astype(np.float32), idx


def candidates(idx, shape, edges, shift):
    """The fused decode: idx int64 [B, k] -> float32 [B, k + 1, 3], float32(e[i] + shift) per axis (one float32 addition), the zero
    translation last."""
    Lx, Ly, Lz = shape
    ex, ey, ez = (np.asarray(e, np.float32) for e in edges)
    s = np.float32(shift)
    ix, iy, iz = idx // (Ly * Lz), idx // Lz % Ly, idx % Lz
    out = np.zeros(idx.shape[:1] + (idx.shape[1] + 1, 3), np.float32)
    out[:, :-1, 0], out[:, :-1, 1], out[:, :-1, 2] = ex[ix] + s, ey[iy] + s, ez[iz] + s
    return out


def parent_z_radii(shape, kernel_size):
    """The z window of the LDS form before its whole-column shortcut was narrowed to Lz <= radius + 1: for
    radius + 1 < Lz <= 2 radius + 1 (and Lz != 3 at radius >= 2, which is right) every bin saw its whole column.
    -> (lo, hi) to hand to peaks(), or None where that form had the right window."""
    r = (int(kernel_size) - 1) // 2
    Lz = shape[2]
    if not (r + 1 < Lz <= 2 * r + 1) or 3 * 4 * int(np.prod(shape)) > 150 * 1024:
        return None
    return (r, r, Lz), (r, r, Lz)

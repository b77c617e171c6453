"""Plain numpy restatement of the trust byte (icpflow_flow_trust, csrc/trust.hip), written from include/icpflow_hip.h, "8(i)
trust byte": one function for the segments' bytes, one for the rows' bytes, one for the sixteen counts.  Shared by
tests/test_trust.py (CPU: held against SegmentResidual.worst and SegmentSight.annotate) and tests/test_gpu_trust.py
(array_equal against the kernels).  Not a test module.

The rules that are the call's own (the header states them):
  * a segment is LISTED iff it is not skipped, has a good row and its AFTER mean EXCEEDS `above` (one fp64 division);
  * "seen through" iff seen > share * far, else "lost from view" iff excused > share * far, else "undecided" (fp64);
  * a row finds its segment by the cluster table's key of its label, a signalling NaN quieted first on both sides;
  * NEAR iff d2 <= (float)far * (float)far in fp32; a bad row is the residual's: |coordinate| <= 1e6 fails (a NaN fails).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_restatement as tr                # noqa: E402

F = np.float32
ROW_MASK, FIT_SHIFT, FIT_MASK = 0x07, 3, 0x03
MATCHED, SKIPPED, KEEP = 0x20, 0x40, 0x80
ROW_BAD, ROW_NEAR, ROW_NO_CODE = 0, 1, 7
ROW_OF_CODE = {2: 2, 3: 3, 4: 4, 1: 5, 0: 6}          # icpflow_sight_query's code of a far row -> ROW
FIT_NAMES = (None, "seen through", "lost from view", "undecided")
DEFAULTS = dict(above=0.1, far=0.1, share=0.5, skip=(-1e8, -1.0))
GOOD_AFTER, SUM_AFTER, FAR_AFTER = 10, 16, 15         # columns of the two tables


def key(labels):
    """float32 labels -> the uint32 keys a row is searched by: the cluster table's, a signalling NaN quieted first"""
    return tr.key(tr.quiet(tr.bits(labels)).view(F))


def segments_of(num, Lmax):
    """the number of segments the kernels work with"""
    return 0 if num <= 0 else min(int(num), int(Lmax))


def segment_bytes(resid, sight, pair_labels, above=0.1, share=0.5, skip=(-1e8, -1.0)):
    """resid float64 [L, 18], sight float64 [L, 24] or None, pair_labels float32 [P] (column 0 of the pair rows)
    -> uint8 [L]: bits 3-6 of every segment"""
    resid = np.asarray(resid, np.float64).reshape(-1, 18)
    L = len(resid)
    label = resid[:, 0]
    pl = np.asarray(pair_labels, F).reshape(-1).astype(np.float64)
    matched = (label[:, None] == pl[None, :]).any(axis=1) if len(pl) else np.zeros(L, bool)     # IEEE ==
    skipped = (label == np.float64(F(skip[0]))) | (label == np.float64(F(skip[1])))
    good, dsum = resid[:, GOOD_AFTER], resid[:, SUM_AFTER]
    with np.errstate(divide="ignore", invalid="ignore"):
        listed = ~skipped & (good != 0.0) & (dsum / good > np.float64(above))
    fit = np.where(listed, 3, 0)
    if sight is not None:
        sight = np.asarray(sight, np.float64).reshape(-1, 24)
        far = np.zeros(L)
        for k in range(5):
            far = far + sight[:, FAR_AFTER + 2 * k]
        seen = sight[:, FAR_AFTER + 4]
        excused = sight[:, FAR_AFTER] + sight[:, FAR_AFTER + 2] + sight[:, FAR_AFTER + 8]
        bar = np.float64(share) * far
        fit = np.where(listed, np.where(seen > bar, 1, np.where(excused > bar, 2, 3)), 0)
    return ((fit << FIT_SHIFT) | np.where(matched, MATCHED, 0) | np.where(skipped, SKIPPED, 0)).astype(np.uint8)


def good_rows(after, flow):
    q = np.asarray(after, F).reshape(-1, 3)
    if flow is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            q = q + np.asarray(flow, F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(q) <= F(1e6)).all(axis=1)


def row_bytes(after, flow, labels, resid, num, segment, d2_after, code_after, far=0.1):
    """-> (trust uint8 [n], has_segment bool [n]); resid [Lmax, 18] (rows from num on are not read), segment uint8 [>= num]"""
    labels = np.asarray(labels, F).reshape(-1)
    n = len(labels)
    resid = np.asarray(resid, np.float64).reshape(-1, 18)
    L = segments_of(num, len(resid))
    with np.errstate(invalid="ignore"):
        keys = key(resid[:L, 0].astype(F))
    want = key(labels)
    at = np.searchsorted(keys, want, side="left")
    found = (at < L) & (keys[np.minimum(at, max(L - 1, 0))] == want) if L else np.zeros(n, bool)
    seg = np.asarray(segment, np.uint8)[np.minimum(at, max(L - 1, 0))].astype(np.int64) if L else np.zeros(n, np.int64)
    good = good_rows(after, flow)
    far2 = F(far) * F(far)
    with np.errstate(invalid="ignore"):
        near = np.asarray(d2_after, F).reshape(-1) <= far2
    row = np.full(n, ROW_NO_CODE, np.int64)
    if code_after is not None:
        code = np.asarray(code_after, np.int32).reshape(-1)
        for c, r in ROW_OF_CODE.items():
            row[code == c] = r
    row[near] = ROW_NEAR
    row[~good] = ROW_BAD
    fit = (seg >> FIT_SHIFT) & FIT_MASK
    keep = (row != ROW_BAD) & (row != 2) & ((fit == 0) | (fit == 2))
    byte = (seg & 0x78) | row | np.where(keep, KEEP, 0)
    return np.where(found, byte, 0).astype(np.uint8), found


def counts(trust, has_segment):
    """-> int64 [16], d_counts"""
    t = np.asarray(trust, np.uint8).astype(np.int64)
    has = np.asarray(has_segment, bool)
    row, fit = t & ROW_MASK, (t >> FIT_SHIFT) & FIT_MASK
    out = np.zeros(16, np.int64)
    for k in range(8):
        out[k] = int((has & (row == k)).sum())
    judged = has & (row != 0) & ((t & SKIPPED) == 0)
    for k in range(4):
        out[8 + k] = int((judged & (fit == k)).sum())
    out[12], out[13], out[14] = int(((t & MATCHED) != 0).sum()), int(((t & SKIPPED) != 0).sum()), int(((t & KEEP) != 0).sum())
    out[15] = int((~has).sum())
    return out


def trust(after, flow, labels, resid, sight, num, d2_after, code_after, pair_labels, above=0.1, far=0.1, share=0.5, skip=(-1e8, -1.0)):
    """the whole call -> dict(trust uint8 [n], segment uint8 [L], counts int64 [16], has_segment bool [n])"""
    resid = np.asarray(resid, np.float64).reshape(-1, 18)
    L = segments_of(num, len(resid))
    seg = segment_bytes(resid[:L], None if sight is None else np.asarray(sight, np.float64).reshape(-1, 24)[:L], pair_labels, above, share, skip)
    t, has = row_bytes(after, flow, labels, resid, num, seg, d2_after, code_after, far)
    return dict(trust=t, segment=seg, counts=counts(t, has), has_segment=has)

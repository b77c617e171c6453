"""Plain numpy restatement of the object tracks across the files of a log (include/icpflow_hip.h, "8(l)": icpflow_rows_carry,
icpflow_pair_row_ids, icpflow_object_tracks_extend_side, icpflow_object_tracks_path; csrc/carry.hip, csrc/tracks.hip), written
from the header's text.  The carry in NumPy float32, operation by operation, over tests/residual_restatement.py's brute-force
search; the ids in integers and np.unique; the path in float64, one Python float operation per operation the header writes
out, in its order.  Not a test module."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_restatement as br             # noqa: E402
import residual_restatement as rr        # noqa: E402
import track_restatement as trk          # noqa: E402

F = np.float32
CARRY_COUNTS, ROW_ID_COUNTS, MAX_PAIRS = 6, 3, 4096
PATH_COLS, PATH_COUNTS = 24, 5
CARRY_RADIUS, CARRY_MIN_SHARE, MAX_DV, MIN_SPEED = 0.02, 0.5, 1.0, 0.5


def moved(prev, pose):
    """the previous rows under the pose narrowed to float32: x' = ((m00 x + m01 y) + m02 z) + m03, each operation a float32
    operation of its own -> (moved float32 [m, 3], good bool [m]: the row and the moved row inside +-1e6 m and finite)"""
    p = np.ascontiguousarray(prev, F).reshape(-1, 3)
    M = np.asarray(pose, np.float64).reshape(4, 4).astype(F)
    out = np.empty_like(p)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = ((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3]
    assert out.dtype == F
    return out, rr.good_rows(p) & rr.good_rows(out)


def rows_carry(prev, prev_id, pose, nxt, radius=CARRY_RADIUS, min_share=CARRY_MIN_SHARE):
    """-> dict(id int32 [n], d2 float32 [n], idx int32 [n], counts int64 [6])"""
    prev_id = np.asarray(prev_id, np.int32).reshape(-1)
    q = np.ascontiguousarray(nxt, F).reshape(-1, 3)
    t, good = moved(prev, pose)
    t = t.copy()
    t[~good] = np.nan                                   # a bad previous row is never a neighbour
    d2, idx, info = rr.search(q, t, None, radius)
    hit = idx >= 0
    ids = np.full(len(q), -1, np.int32)
    ids[hit] = prev_id[idx[hit]]
    ids[ids < 0] = -1
    counts = np.array([hit.sum(), (ids >= 0).sum(), (idx == -1).sum(), info["bad_queries"], int((~good).sum()), 0], np.int64)
    if float(counts[0]) < float(min_share) * float(len(q)):
        counts[5] = 1
        ids[:] = -1
    return dict(id=ids, d2=d2, idx=idx, counts=counts)


def pair_row_ids(labels, pair_rows, col, pair_id, weight=None):
    """-> (ids int32 [n], counts int64 [3]): per key the pair with an id >= 0 and the largest weight (a NaN weighs least), the
    lowest p among equals"""
    labels = np.asarray(labels, F).reshape(-1)
    pair_id = np.asarray(pair_id, np.int32).reshape(-1)
    P = len(pair_id)
    pairs = np.asarray(pair_rows, F).reshape(P, -1) if P else np.zeros((0, 2), F)
    w = np.zeros(P) if weight is None else np.asarray(weight, np.float64).reshape(P).copy()
    w[np.isnan(w)] = -np.inf
    keys = np.array([br.label_key(v) for v in pairs[:, col]], np.int64)
    winner, shared = {}, 0
    uniq, first = np.unique(keys, return_index=True)
    shared = P - len(uniq)
    for k in uniq:
        mine = np.flatnonzero((keys == k) & (pair_id >= 0))
        if len(mine):
            winner[int(k)] = int(pair_id[mine[np.argmax(w[mine])]])      # (the first maximum: the lowest p)
    ids = np.full(len(labels), -1, np.int32)
    for i, v in enumerate(labels):
        if not (v < 0):
            ids[i] = winner.get(br.label_key(v), -1)
    return ids, np.array([(ids >= 0).sum(), (ids < 0).sum(), shared], np.int64)


def swapped(objects):
    """object rows with the two label columns exchanged: side 0 on them is side 1 on the originals"""
    if objects is None:
        return None
    o = np.asarray(objects, np.float64).reshape(-1, br.OBJECT_COLS).copy()
    o[:, [0, 1]] = o[:, [1, 0]]
    return o


def extend_side(labels, track_of_row, next_id, objects, side, gap, seconds, min_iou=trk.MIN_IOU, Lmax=4096):
    return trk.extend(labels, track_of_row, next_id, objects if side == 1 else swapped(objects), gap, seconds, min_iou, Lmax)


def frames_chain(poses):
    """W_0 = I, W_{k+1} = W_k inverse(pose_{k+1}) in float64, the inverse of a rigid pose (R, t) being (R^T, -R^T t)
    -> float64 [F, 12]: the rotation row-major, then the translation"""
    W = np.eye(4)
    out = []
    for k, pose in enumerate(poses):
        if k > 0:
            P = np.asarray(pose, np.float64).reshape(4, 4)
            inv = np.eye(4)
            inv[:3, :3] = P[:3, :3].T
            inv[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
            W = W @ inv
        out.append(np.concatenate([W[:3, :3].reshape(9), W[:3, 3]]))
    return np.array(out).reshape(len(poses), 12)


def path(obs, step, frames, T, max_dv=MAX_DV, min_speed=MIN_SPEED):
    """-> (paths float64 [T, 24], counts int64 [5])"""
    obs = np.asarray(obs, np.float64).reshape(-1, trk.OBS_COLS)
    step = np.asarray(step, np.int64).reshape(-1)
    frames = np.asarray(frames, np.float64).reshape(-1, 12)
    Fn = len(frames)
    out, counts = np.zeros((T, PATH_COLS)), np.zeros(PATH_COUNTS, np.int64)
    counts[0] = T
    for t in range(T):
        counted, cand = [], None                         # (row, step) of the observations that count
        for k in range(len(obs)):
            if obs[k, 0] != float(t) or not (0 <= step[k] < Fn):
                continue
            if cand is not None and step[k] == cand[1]:
                if obs[k, 9] > obs[cand[0], 9]:
                    cand = (k, int(step[k]))
                continue
            if cand is not None:
                counted.append(cand)
            cand = (k, int(step[k]))
        if cand is not None:
            counted.append(cand)
        seconds, length, total = 0.0, 0.0, [0.0, 0.0, 0.0]
        dv_max, jump_max, pairs = 0.0, 0.0, 0
        sizes, start, prev = [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], None
        with np.errstate(all="ignore"):
            for k, s in counted:
                o, f = [float(x) for x in obs[k]], [float(x) for x in frames[s]]
                c = [((f[3 * r] * o[10] + f[3 * r + 1] * o[11]) + f[3 * r + 2] * o[12]) + f[9 + r] for r in range(3)]
                d = [(f[3 * r] * o[3] + f[3 * r + 1] * o[4]) + f[3 * r + 2] * o[5] for r in range(3)]
                v = [float(np.float64(d[r]) / np.float64(o[2])) for r in range(3)]
                if prev is None:
                    start = c
                elif s == prev[0] + 1:
                    ax, ay = v[0] - prev[3][0], v[1] - prev[3][1]
                    dv = math.sqrt(ax * ax + ay * ay)
                    jx, jy = (prev[1][0] + prev[2][0]) - c[0], (prev[1][1] + prev[2][1]) - c[1]
                    jump = math.sqrt(jx * jx + jy * jy)
                    dv_max, jump_max = (dv if dv > dv_max else dv_max), (jump if jump > jump_max else jump_max)
                    pairs += 1
                seconds = seconds + o[2]
                length = length + math.sqrt(d[0] * d[0] + d[1] * d[1])
                for r in range(3):
                    total[r] = total[r] + d[r]
                for j in range(4):
                    sizes[j] = o[6 + j] if o[6 + j] > sizes[j] else sizes[j]
                prev = (s, c, d, v)
            mean = [float(np.float64(total[r]) / np.float64(seconds)) for r in range(3)] if counted else [0.0, 0.0, 0.0]
        speed = math.sqrt(mean[0] * mean[0] + mean[1] * mean[1])
        observed = bool(counted)
        moving = observed and speed >= min_speed
        judged = pairs >= 1
        smooth = judged and dv_max <= max_dv
        first, last = (counted[0][1], counted[-1][1]) if counted else (0, 0)
        out[t] = [t, len(counted), first, last, (last - first + 1) - len(counted) if counted else 0, seconds, length, mean[0], mean[1], mean[2], speed,
                  dv_max, pairs, jump_max, moving, judged, smooth] + sizes + start
        counts[1:] += [observed, judged, smooth, moving]
    return out, counts

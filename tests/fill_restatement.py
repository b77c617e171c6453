"""The track fill (include/icpflow_hip.h, "8(n) track fill") restated in NumPy, one operation per operation of the header:
`missing` is icpflow_object_tracks_missing, `candidates` is icpflow_pairs_fill_candidates (its label comparison in float32, its
fp64 sums in the header's order), `append` is the bookkeeping of pair_judges.frame_tracks(fill=True) -- which rows the new
tensors gain and that no old row changes.  Plain loops, no GPU, nothing of the package imported.  Not a test module."""
import numpy as np

F = np.float32
OBS_COLS, SEGMENT_COLS, BOX_COLS = 13, 6, 16
MISSING_COLS, MISSING_COUNTS, MAX_SLOTS, CHOICE_COLS, FILL_COUNTS = 14, 4, 64, 8, 4
MAX_RESIDUAL, FILL_RADIUS = 0.2, 1.0
CHOSEN, NONE, LOST = 0, 1, 2
POISON = np.float64(-7.25)                         # what `missing` leaves in the rows the header says are not written


def missing(obs, T, segments, num, gaps, seconds, max_residual=MAX_RESIDUAL):
    """obs [M, 13]; segments [G, Lmax, 6]; num [G]; gaps, seconds [G] -> (plan float64 [G, Lmax, 14], written bool [G, Lmax],
    counts int64 [G, 4]); the rows that are not written hold POISON"""
    obs = np.asarray(obs, np.float64).reshape(-1, OBS_COLS)
    segments = np.asarray(segments, np.float64)
    G, Lmax = segments.shape[0], segments.shape[1]
    M = len(obs)
    plan, written, counts = np.full((G, Lmax, MISSING_COLS), POISON), np.zeros((G, Lmax), bool), np.zeros((G, MISSING_COUNTS), np.int64)
    m2 = np.float64(max_residual) * np.float64(max_residual)
    for g in range(G):
        for c in range(min(int(num[g]), Lmax)):
            seg = segments[g, c]
            t = seg[2]
            row = np.zeros(MISSING_COLS)
            row[1], row[2], row[13] = t, seg[0], seg[1]
            written[g, c] = True
            plan[g, c] = row
            if not (t >= 0.0 and t < float(T)):
                continue
            counts[g, 0] += 1
            A, B, L, mask, others, observed, rows = np.float64(0.0), np.zeros(3), np.zeros(3), 0, 0, 0, []
            with np.errstate(all="ignore"):
                for i in range(M):
                    if obs[i, 0] != t:
                        continue
                    if obs[i, 1] == float(gaps[g]):
                        observed += 1
                        continue
                    s = obs[i, 2]
                    A = A + s * s
                    for a in range(3):
                        B[a] = B[a] + s * obs[i, 3 + a]
                        L[a] = L[a] + (obs[i, 10 + a] + obs[i, 3 + a])
                    if 0.0 <= obs[i, 1] < 64.0:
                        mask |= 1 << int(obs[i, 1])
                    others += 1
                    rows.append(i)
                distinct = bin(mask).count("1")
                row[3], row[4], row[5] = observed, others, distinct
                plan[g, c] = row
                if observed:
                    continue
                counts[g, 1] += 1
                if not (distinct >= 2 and A > 0.0):
                    continue
                counts[g, 2] += 1
                v = B / A
                inner = np.float64(0.0)
                for i in rows:
                    rx, ry = obs[i, 3] - obs[i, 2] * v[0], obs[i, 4] - obs[i, 2] * v[1]
                    r2 = rx * rx + ry * ry
                    inner = r2 if r2 > inner else inner
                p = np.float64(seconds[g]) * v
                q = L / np.float64(others) - p
                miss = bool(inner <= m2)
                counts[g, 3] += miss
                row[0], row[6:9], row[9:12], row[12] = float(miss), p, q, np.sqrt(inner)
            plan[g, c] = row
    return plan, written, counts


def _d2(box, q):
    with np.errstate(all="ignore"):
        dx, dy = box[6] - q[0], box[7] - q[1]
        return dx * dx + dy * dy


def is_candidate(boxes, num_src, pair_labels, max_rows):
    """-> bool [L]: has a box, short enough, its label (narrowed to float) equal to no matched source label (IEEE ==)"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, BOX_COLS)
    L = max(0, min(int(num_src), len(boxes)))
    taken = np.asarray(pair_labels, F).reshape(-1)
    out = np.zeros(L, bool)
    for c in range(L):
        label = F(boxes[c, 0])
        with np.errstate(all="ignore"):
            out[c] = bool(boxes[c, 3] >= 0.0) and bool(boxes[c, 1] <= float(max_rows)) and not bool((taken == label).any())
    return out


def candidates(q, boxes, num_src, pair_labels, radius=FILL_RADIUS, max_rows=10000):
    """q [K, 3]; boxes [Lmax, 16]; pair_labels [P]: column 0 of the pair rows -> (choice float64 [K, 8], counts int64 [4])"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    boxes = np.asarray(boxes, np.float64).reshape(-1, BOX_COLS)
    K = len(q)
    choice, counts = np.zeros((K, CHOICE_COLS)), np.zeros(FILL_COUNTS, np.int64)
    if K == 0:
        return choice, counts
    cand = is_candidate(boxes, num_src, pair_labels, max_rows)
    counts[3] = cand.sum()
    r2 = np.float64(radius) * np.float64(radius)
    best = []
    for k in range(K):
        d2, at = None, -1
        for c in np.flatnonzero(cand):
            d = _d2(boxes[c], q[k])
            if bool(d <= r2) and (at < 0 or d < d2):
                d2, at = d, int(c)
        best.append((d2, at))
        if at < 0:
            choice[k, 0], choice[k, 1] = NONE, -1.0
        else:
            choice[k] = [CHOSEN, at, boxes[at, 0], boxes[at, 1], np.sqrt(d2), boxes[at, 6], boxes[at, 7], boxes[at, 8]]
    for k, (d2, at) in enumerate(best):
        if at >= 0 and any(a == at and (d < d2 or (d == d2 and j < k)) for j, (d, a) in enumerate(best) if j != k):
            choice[k, 0] = LOST
    for r in (CHOSEN, NONE, LOST):
        counts[r] = int((choice[:, 0] == r).sum())
    return choice, counts


def append(pairs, transformations, labels, metrics, T_new, accepted):
    """The bookkeeping of a filled gap.  pairs float32 [P, 10], transformations float32 [P, 4, 4]; per retried row, in ascending
    plan-row order: labels [K, 2] (the chosen source label, the plan's destination label), metrics: dict of the new errors,
    inliers, ratios, ious [K, 2], T_new [K, 4, 4], accepted bool [K].  -> (pairs [P + a, 10], transformations [P + a, 4, 4]): the
    accepted rows appended in that order, every old row as it was"""
    pairs, transformations = np.array(pairs, F).reshape(-1, 10), np.array(transformations, F).reshape(-1, 4, 4)
    rows, Ts = [], []
    for k in np.flatnonzero(np.asarray(accepted, bool)):
        rows.append(np.concatenate([np.asarray(labels, F)[k]] + [np.asarray(metrics[name], F)[k] for name in ("errors", "inliers", "ratios", "ious")]))
        Ts.append(np.asarray(T_new, F).reshape(-1, 4, 4)[k])
    if not rows:
        return pairs, transformations
    return np.concatenate([pairs, np.array(rows, F)]), np.concatenate([transformations, np.array(Ts, F)])

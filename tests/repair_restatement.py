"""The track repair (include/icpflow_hip.h, "8(m) track repair") restated in NumPy, one operation per operation of the header:
`plan` is icpflow_object_tracks_suspects, `select` is icpflow_pairs_repair_select (its float32 comparisons in float32, its
fp64 sums in the header's order), `patch` is the bookkeeping of pair_judges.frame_tracks(repair=True) -- which transforms, which
columns of the pair rows and which flow rows change.  Plain loops, no GPU, nothing of the package imported.  Not a test module."""
import numpy as np

F = np.float32
OBS_COLS, PLAN_COLS, PLAN_COUNTS, REPAIR_COLS, REPAIR_COUNTS = 13, 8, 4, 12, 8
MAX_RESIDUAL = 0.2
DEFAULTS = dict(translation_frame=2.0, thres_iou=0.2, rot_limit_deg=9.0, thres_error=0.2, max_residual=0.2)
ACCEPTED, REJECT_TEST, ERROR, OFF_PREDICTION, NOT_BETTER, ABANDONED, TOO_LONG = 0, 1, 2, 3, 4, 5, 6


def plan(obs, T, max_residual=MAX_RESIDUAL):
    """-> (plan float64 [M, 8], counts int64 [4])"""
    obs = np.asarray(obs, np.float64).reshape(-1, OBS_COLS)
    M = len(obs)
    out, counts = np.zeros((M, PLAN_COLS)), np.zeros(PLAN_COUNTS, np.int64)
    m2 = np.float64(max_residual) * np.float64(max_residual)
    for j in range(M):
        t = obs[j, 0]
        if not (t >= 0.0 and t < float(T)):
            continue
        counts[0] += 1
        A, B, mask, others = np.float64(0.0), np.zeros(3), 0, 0
        rows = [i for i in range(M) if i != j and obs[i, 0] == t]
        for i in rows:
            s = obs[i, 2]
            A = A + s * s
            for a in range(3):
                B[a] = B[a] + s * obs[i, 3 + a]
            if 0.0 <= obs[i, 1] < 64.0:
                mask |= 1 << int(obs[i, 1])
            others += 1
        gaps = bin(mask).count("1")
        out[j, 1], out[j, 2] = others, gaps
        if not (gaps >= 2 and A > 0.0):
            continue
        counts[1] += 1
        with np.errstate(all="ignore"):
            v = B / A
            inner = np.float64(0.0)
            for i in rows:
                rx, ry = obs[i, 3] - obs[i, 2] * v[0], obs[i, 4] - obs[i, 2] * v[1]
                r2 = rx * rx + ry * ry
                inner = r2 if r2 > inner else inner
            p = obs[j, 2] * v
            rx, ry = obs[j, 3] - p[0], obs[j, 4] - p[1]
            r2 = rx * rx + ry * ry
            agreed = bool(inner <= m2)
            suspect = agreed and bool(r2 > m2)
            counts[2] += agreed
            counts[3] += suspect
            out[j, 0], out[j, 3:6], out[j, 6], out[j, 7] = float(suspect), p, np.sqrt(r2), np.sqrt(inner)
    return out, counts


def _min_error(e):
    """min(error_src, error_dst) in float32, NaN if either is"""
    e = np.asarray(e, F)
    return F(np.nan) if (np.isnan(e[0]) or np.isnan(e[1])) else (e[0] if e[0] < e[1] else e[1])


def reject_test(errors, ious, translations, rotations, tf, thres_iou, rot_limit):
    """check_transformation of one pair in float32 as the association evaluates it -> (keep, nrm, iou, angle)"""
    t, iou, rot = np.asarray(translations, F), np.asarray(ious, F), np.asarray(rotations, F)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(F(F(t[0] * t[0]) + F(t[1] * t[1])) + F(t[2] * t[2]), dtype=F)
        low = iou[1] if iou[1] < iou[0] else iou[0]
        angle = np.fmax(np.abs(rot[1]), np.abs(rot[2]))
        far = bool(nrm > F(tf))
        low_iou = bool(low < F(thres_iou))
        turned = (not np.isnan(rot[1]) and not np.isnan(rot[2])) and bool(angle > F(rot_limit))
    return (not far and not low_iou and not turned), F(nrm), F(low), F(angle)


def displacement(T, c):
    """d = T c - c in fp64 in the order of icpflow_pair_objects' columns 7-9"""
    m, c = np.asarray(T, F).reshape(16).astype(np.float64), np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        return np.array([(((m[4 * a] * c[0] + m[4 * a + 1] * c[1]) + m[4 * a + 2] * c[2]) + m[4 * a + 3]) - c[a] for a in range(3)])


def select(T_new, T_old, iters, errors, ious, translations, rotations, errors_old, centre, pred, **params):
    """-> (T_out float32 [K, 16], report float64 [K, 12], counts int64 [8])"""
    p = dict(DEFAULTS, **params)
    T_new, T_old = np.asarray(T_new, F).reshape(-1, 16), np.asarray(T_old, F).reshape(-1, 16)
    K = len(T_new)
    errors, ious, errors_old = (np.asarray(x, F).reshape(K, 2) for x in (errors, ious, errors_old))
    translations, rotations = (np.asarray(x, F).reshape(K, 3) for x in (translations, rotations))
    centre, pred = (np.asarray(x, np.float64).reshape(K, 3) for x in (centre, pred))
    out, report, counts = np.empty((K, 16), F), np.zeros((K, REPAIR_COLS)), np.zeros(REPAIR_COUNTS, np.int64)
    m2 = np.float64(p["max_residual"]) * np.float64(p["max_residual"])
    for k in range(K):
        keep, nrm, iou, angle = reject_test(errors[k], ious[k], translations[k], rotations[k], p["translation_frame"], p["thres_iou"], p["rot_limit_deg"])
        e_new, e_old = _min_error(errors[k]), _min_error(errors_old[k])
        d = displacement(T_new[k], centre[k])
        with np.errstate(all="ignore"):
            qx, qy = d[0] - pred[k, 0], d[1] - pred[k, 1]
            q2 = qx * qx + qy * qy
            if int(iters) < 0:
                reason = ABANDONED
            elif not keep:
                reason = REJECT_TEST
            elif np.isnan(e_new) or not bool(e_new < F(p["thres_error"])):
                reason = ERROR
            elif bool(q2 > m2):
                reason = OFF_PREDICTION
            elif not np.isnan(e_old) and bool(e_new > e_old):
                reason = NOT_BETTER
            else:
                reason = ACCEPTED
            out[k] = T_new[k] if reason == ACCEPTED else T_old[k]
            report[k] = [reason, e_new, e_old, d[0], d[1], d[2], np.sqrt(q2), int(iters), iou, nrm, angle, float(reason == ACCEPTED)]
        counts[reason] += 1
    return out, report, counts


def flow_rows(points, T, pose=None):
    """icpflow_flow_rigid_rows' arithmetic for the rows of one cluster: float32, moved = (T pose) p, flow = moved - p -- used only to
    say WHICH rows change; the numbers are compared against the device's own wrapper"""
    M = np.asarray(T, np.float64).reshape(4, 4) @ (np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4))
    p = np.asarray(points, np.float64)
    return ((p @ M[:3, :3].T + M[:3, 3]) - p).astype(F)


def patch(pairs, transformations, labels_src, retried, T_out, report, metrics):
    """The bookkeeping of a repaired gap.  pairs float32 [P, 10], transformations float32 [P, 4, 4], labels_src [n] the source labels
    of the gap's points, retried: the pair rows that were registered again, T_out / report: the select's, metrics: dict of the
    new errors, inliers, ratios, ious [K, 2].  -> (pairs, transformations, the mask of the flow rows that change): only accepted
    pairs change -- their transform, columns 2-9 of their pair row, the flow rows of their source label."""
    pairs, transformations = np.array(pairs, F), np.array(transformations, F).reshape(-1, 4, 4)
    changed = np.zeros(len(np.asarray(labels_src)), bool)
    for k, row in enumerate(retried):
        if report[k, 11] != 1.0:
            continue
        transformations[row] = np.asarray(T_out[k], F).reshape(4, 4)
        for c, name in enumerate(("errors", "inliers", "ratios", "ious")):
            pairs[row, 2 + 2 * c: 4 + 2 * c] = np.asarray(metrics[name], F)[k]
        changed |= np.asarray(labels_src, F) == pairs[row, 0]
    return pairs, transformations, changed

"""The host half of an association stage, restated in plain numpy (no GPU, no package import): what icpflow_assoc_assign and
icpflow_assoc_collect (csrc/assoc.hip) must compute, bit for bit.

Reference: match_pairs' loop (utils_match.py:96-115) with check_transformation (utils_check.py:51-66) and the row arg-min
(utils_helper.py:108-110), and match_pcds' step from stage 1 to stage 2 (utils_match.py:42-53).

Two statements of the assignment live here:

  * `assign`      -- the LIST form: one pass over the candidates, what the kernel does;
  * `assign_loop` -- the reference's own loop on torch scalars and S x D matrices (torch.linalg.norm, builtin min, a 1e8-filled
                     [S,D,2] matrix, .min(-1), torch.argmin).  tests/test_association_restatement.py pins the first to the second.

`random_stage` is the generator both the CPU and the GPU test draw from, and `Branches` counts, over a run, how often each rule
of the statement DECIDED a row -- so that a test cannot pass by never entering a branch.

A stage's results are one flat float32 buffer, array after array (include/icpflow_hip.h):
    [T 16K | errors 2K | inliers 2K | ratios 2K | ious 2K | translations 3K | rotations 3K | iteration count (int32)]
"""
from types import SimpleNamespace

import numpy as np

F = np.float32


def _nx(x, up=True):
    return np.nextafter(F(x), F(np.inf) if up else F(-np.inf))


# (translation_frame, thres_iou, thres_rot * 90, thres_error): float32-representable where it matters, so that comparing a
# float32 value with the float32 or with the double threshold gives the same answer
PARAMS = SimpleNamespace(tf=F(2.5), thres_iou=F(0.2), rot_limit=F(9.0), thres_error=F(0.2))

# the statement with ONE rule replaced by a plausible wrong one: a row whose outcome differs was decided by that rule
VARIANTS = ("nan_translation_rejects", "iou_minimum_propagates", "iou_fmin_drops", "rot_fmax_drops", "nan_error_dropped")


def unpack(result, K):
    """Views into the flat result buffer of a stage of K candidates."""
    r = np.asarray(result, F)
    assert r.shape == (30 * K + 1,)
    f = SimpleNamespace(T=r[:16 * K].reshape(K, 16), errors=r[16 * K:18 * K].reshape(K, 2), inliers=r[18 * K:20 * K].reshape(K, 2),
                        ratios=r[20 * K:22 * K].reshape(K, 2), ious=r[22 * K:24 * K].reshape(K, 2),
                        translations=r[24 * K:27 * K].reshape(K, 3), rotations=r[27 * K:30 * K].reshape(K, 3))
    f.iters = int(r[30 * K:].view(np.int32)[0])
    return f


def pack(T, errors, inliers, ratios, ious, translations, rotations, iters=7):
    parts = [np.asarray(a, F).reshape(-1) for a in (T, errors, inliers, ratios, ious, translations, rotations)]
    return np.concatenate(parts + [np.array([iters], np.int32).view(F)])


def reject_reasons(params, f, variant=None):
    """check_transformation (utils_check.py:51-66) per candidate -> (far_off, low_iou, turned), each bool [K]."""
    t = f.translations
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        far = nrm > params.tf
        if variant == "nan_translation_rejects":
            far |= np.isnan(nrm)
        i0, i1 = f.ious[:, 0], f.ious[:, 1]
        mn = np.where(i1 < i0, i1, i0)                       # Python's builtin min(iou), utils_match.py:99
        if variant == "iou_minimum_propagates":
            mn = np.minimum(i0, i1)
        if variant == "iou_fmin_drops":
            mn = np.fmin(i0, i1)
        low = mn < params.thres_iou
        r1, r2 = np.abs(f.rotations[:, 1]), np.abs(f.rotations[:, 2])
        turned = (np.fmax(r1, r2) if variant == "rot_fmax_drops" else np.maximum(r1, r2)) > params.rot_limit
    return far, low, turned


def keep_mask(params, f, active, variant=None):
    far, low, turned = reject_reasons(params, f, variant)
    keep = ~far & ~low & ~turned
    if active is not None:
        keep &= np.asarray(active) != 0
    return keep


def assign(params, S, D, si, di, active, result, variant=None):
    """-> best int32 [S]: per source row the index of its matched candidate, or -1."""
    si, di = np.asarray(si), np.asarray(di)
    K = len(si)
    assert K > 0 and si.min() >= 0 and si.max() < S and di.min() >= 0 and di.max() < D
    f = unpack(result, K)
    keep = keep_mask(params, f, active, variant)
    with np.errstate(invalid="ignore"):
        err = np.minimum(f.errors[:, 0], f.errors[:, 1])    # NaN if either is
    if variant == "nan_error_dropped":
        keep &= ~np.isnan(err)
    best = np.full(S, -1, np.int32)
    kept = np.nonzero(keep)[0]
    for s in np.unique(si[kept]):
        ks = kept[si[kept] == s]
        if np.isnan(err[ks]).any():                          # argmin takes the NaN, and NaN < thres_error is false
            continue
        k = ks[np.lexsort((di[ks], err[ks]))[0]]             # smallest error, ties to the smallest destination row
        if err[k] < params.thres_error:
            best[s] = k
    return best


def assign_loop(params, S, D, si, di, active, result):
    """The reference's own loop (utils_match.py:96-115, utils_check.py:51-66, utils_helper.py:108-110) on torch scalars."""
    import torch
    K = len(si)
    f = unpack(result, K)
    tf, thres_iou, max_rot, thres_error = (float(params.tf), float(params.thres_iou), float(params.rot_limit),
                                           float(params.thres_error))
    errors, ious = torch.from_numpy(f.errors.copy()), torch.from_numpy(f.ious.copy())
    translations, rotations = torch.from_numpy(f.translations.copy()), torch.from_numpy(f.rotations.copy())
    m_err = torch.zeros((S, D, 2)) + 1e8
    index = np.full((S, D), -1, np.int64)
    n_kept = 0
    for k in range(K):
        if active is not None and not active[k]:
            continue
        if torch.linalg.norm(translations[k]) > tf:
            continue
        if min(ious[k]) < thres_iou:
            continue
        if torch.abs(rotations[k][1:3]).max() > max_rot:
            continue
        m_err[int(si[k]), int(di[k]), :] = errors[k]
        index[int(si[k]), int(di[k])] = k
        n_kept += 1
    best = np.full(S, -1, np.int32)
    if n_kept > 0:
        row_min, _ = m_err.min(-1)
        rows_s = torch.arange(0, S)
        cols_d = torch.argmin(row_min, dim=1)
        valid = (row_min[rows_s, cols_d] < thres_error).numpy()
        d = cols_d.numpy()
        for s in range(S):
            if valid[s]:
                best[s] = index[s, d[s]]
    return best


def switch(best, si, di, D, si2, di2, seg2):
    """Stage 1 -> stage 2 (utils_match.py:45-53): a stage-2 candidate is on only if neither its source row nor its
    destination row is matched by stage 1.  -> active2 uint8 [K2], seg2 int64 [2,3,K2] with the LENGTHS (row 1 of either
    cloud) of the switched-off candidates set to 0 and every other word as it was."""
    best, si, di = np.asarray(best), np.asarray(si), np.asarray(di)
    mS = best >= 0
    mD = np.zeros(D, bool)
    mD[di[best[mS]]] = True
    on = ~mS[np.asarray(si2)] & ~mD[np.asarray(di2)]
    out = np.array(seg2, np.int64, copy=True).reshape(2, 3, len(si2))
    out[0, 1, ~on] = 0
    out[1, 1, ~on] = 0
    return on.astype(np.uint8), out


FILL_LABEL = F(-3.0e38)


def collect(best1, stage1, best2, stage2, src_labels, dst_labels, cap):
    """The pair rows of both stages, stage 1 first, each in ascending source row -> rows float32 [cap,10], T float32 [cap,16],
    count.  stage = (si, di, result); stage2 / best2 may be None.  Labels: float64 per table row, cast to float32."""
    rows = np.zeros((cap, 10), F)
    rows[:, 0:2] = FILL_LABEL
    T = np.tile(np.eye(4, dtype=F).reshape(1, 16), (cap, 1))
    P, abandoned = 0, False
    for best, stage in ((best1, stage1), (best2, stage2)):
        if stage is None or best is None:
            continue
        si, di, result = stage
        f = unpack(result, len(si))
        abandoned |= f.iters < 0
        for s in range(len(best)):
            k = int(best[s])
            if k < 0:
                continue
            if P < cap:
                with np.errstate(over="ignore"):
                    rows[P, 0], rows[P, 1] = F(src_labels[s]), F(dst_labels[di[k]])
                # (bit for bit: no arithmetic on the copied words)
                rows[P, 2:10].view(np.uint32)[:] = np.concatenate([f.errors[k], f.inliers[k], f.ratios[k], f.ious[k]]).view(np.uint32)
                T[P].view(np.uint32)[:] = f.T[k].view(np.uint32)
            P += 1
    return rows, T, (-1 if abandoned else min(P, cap))


# ---------------------------------------------------------------------------------------------------------- the generator
# whole translation vectors, so that every correct evaluation order of the norm agrees on which side of tf = 2.5 they lie
_T_NEAR = [(0, 0, 0), (0.5, -1.0, 0), (0, 0, 2.5), (1.5, 2.0, 0), (0, -2.0, 1.5), (2.0, 0, -1.5), (0, _nx(2.5, False), 0),
           (-2.5, 0, 0), (0.25, 0.5, -0.5)]
_T_FAR = [(0, 0, _nx(2.5)), (0, -_nx(2.5), 0), (3.0, 0, 0), (2.0, 2.0, 0), (0, 0, np.inf), (-2.0, 1.5, 1.0)]
_IOU_OK = [0.2, _nx(0.2), 0.5, 0.9, 1.0]
_IOU_LOW = [_nx(0.2, False), 0.1, 0.0]
_ROT_OK = [0.0, -3.0, 9.0, -9.0, _nx(9.0, False), 0.5]
_ROT_BAD = [_nx(9.0), -_nx(9.0), 40.0, -170.0]
_ERR_LOW = [0.03, 0.05, 0.1, 0.15, _nx(0.2, False)]
_ERR_HIGH = [0.2, _nx(0.2), 0.3, np.inf, 5.0e8]


def _draw(rng, good, bad, p_bad, size):
    g = np.asarray(good, F)[rng.integers(0, len(good), size)]
    b = np.asarray(bad, F)[rng.integers(0, len(bad), size)]
    return np.where(rng.random(size) < p_bad, b, g).astype(F)


def random_cells(rng, S, D, K):
    """K distinct (source, destination) cells in random candidate order."""
    cells = rng.choice(S * D, K, replace=False) if S * D > 4 * K else rng.permutation(S * D)[:K]
    return (cells // D).astype(np.int32), (cells % D).astype(np.int32)


def random_stage(rng, S, D, K=None, cells=None, mode="mixed", active="random", nan_rate=0.02, iters=7):
    """One stage with ties, NaNs in each of the six arrays, infinite errors, values exactly on each threshold and one float32
    ulp beyond it.  mode: 'mixed' | 'rejected' (no candidate survives) | 'high' (errors at or above thres_error only);
    active: None (no mask) | 'ones' | 'random' | 'zeros'."""
    if cells is None:
        if K is None:
            K = int(rng.integers(1, S * D + 1)) if rng.random() < 0.15 else int(rng.integers(1, min(S * D, 3 * max(S, D)) + 1))
        cells = random_cells(rng, S, D, K)
    si, di = (np.ascontiguousarray(c, np.int32) for c in cells)
    K = len(si)
    p_high = {"mixed": 0.3, "rejected": 0.3, "high": 1.0}[mode]
    errors = _draw(rng, _ERR_LOW, _ERR_HIGH, p_high, (K, 2))
    far = rng.random(K) < (1.0 if mode == "rejected" else 0.08)
    tn = np.asarray(_T_NEAR, F)[rng.integers(0, len(_T_NEAR), K)]
    tfar = np.asarray(_T_FAR, F)[rng.integers(0, len(_T_FAR), K)]
    translations = np.where(far[:, None], tfar, tn).astype(F)
    ious = _draw(rng, _IOU_OK, _IOU_LOW, 0.06, (K, 2))
    rotations = _draw(rng, _ROT_OK, _ROT_BAD, 0.05, (K, 3))
    rotations[:, 0] = _draw(rng, [0.0, 90.0, -179.0, 12.0], [np.nan], 0.1, K)       # yaw: never read
    inliers = rng.integers(0, 500, (K, 2)).astype(F)
    ratios = rng.random((K, 2)).astype(F)
    for a in (errors, inliers, ratios, ious, translations, rotations):
        a[rng.random(a.shape) < nan_rate] = np.nan
    # a NaN beside a value that fails the test on its own: where min / max that DROP or PROPAGATE a NaN part ways
    for col in (0, 1):
        m = rng.random(K) < 1.5 * nan_rate
        ious[m, col], ious[m, 1 - col] = np.nan, F(0.1)
        m = rng.random(K) < 1.5 * nan_rate
        rotations[m, 1 + col], rotations[m, 2 - col] = np.nan, F(40.0)
    T =rng.integers(0, 1 << 32, (K, 16), dtype=np.uint64).astype(np.uint32).view(F)   # any bit pattern, NaN payloads included
    act = {None: None, "ones": np.ones(K, np.uint8), "zeros": np.zeros(K, np.uint8),
           "random": (rng.random(K) < 0.85).astype(np.uint8)}[active]
    return SimpleNamespace(S=S, D=D, K=K, si=si, di=di, active=act,
                           result=pack(T, errors, inliers, ratios, ious, translations, rotations, iters))


def stage_plan(trial):
    """(mode, active) of the trial-th random stage of a run: mostly mixed, with the rare whole-stage cases at fixed trials."""
    if trial % 50 == 17:
        return "mixed", "zeros"
    if trial % 50 == 33:
        return "rejected", "ones"
    mode = "high" if trial % 5 == 2 else "mixed"
    return mode, (None, "ones", "random", "random")[trial % 4]


def plain_stage(S, D, si, di, err=0.1):
    """Every candidate passes every test with the same error (for cases built by hand)."""
    K = len(si)
    T = np.tile(np.eye(4, dtype=F).reshape(1, 16), (K, 1)) + np.arange(K, dtype=F)[:, None]
    return SimpleNamespace(S=S, D=D, K=K, si=np.asarray(si, np.int32), di=np.asarray(di, np.int32), active=None,
                           result=pack(T, np.full((K, 2), err, F), np.full((K, 2), 100, F), np.full((K, 2), 0.9, F),
                                       np.full((K, 2), 0.8, F), np.zeros((K, 3), F), np.zeros((K, 3), F)))


class Branches:
    """Over a run: how often each rule of the statement decided something."""

    def __init__(self):
        self.alone = {"far_off": 0, "low_iou": 0, "turned": 0}
        self.decided = dict.fromkeys(VARIANTS, 0)
        self.tie_not_first = 0
        self.threshold_only = 0
        self.stages_nothing_kept = 0
        self.stages_all_inactive = 0
        self.stages = 0

    def count(self, params, st, best):
        f = unpack(st.result, st.K)
        act = np.ones(st.K, bool) if st.active is None else st.active != 0
        far, low, turned = reject_reasons(params, f)
        self.alone["far_off"] += int((act & far & ~low & ~turned).sum())
        self.alone["low_iou"] += int((act & ~far & low & ~turned).sum())
        self.alone["turned"] += int((act & ~far & ~low & turned).sum())
        for v in VARIANTS:
            self.decided[v] += int((assign(params, st.S, st.D, st.si, st.di, st.active, st.result, variant=v) != best).sum())
        keep = keep_mask(params, f, st.active)
        with np.errstate(invalid="ignore"):
            err = np.minimum(f.errors[:, 0], f.errors[:, 1])
        kept = np.nonzero(keep)[0]
        for s in np.unique(st.si[kept]):
            ks = kept[st.si[kept] == s]
            if np.isnan(err[ks]).any():
                continue
            if best[s] < 0:
                self.threshold_only += 1          # candidates survived, no NaN: only thres_error stands between the winner and a match
            else:
                tied = ks[err[ks] == err[best[s]]]
                self.tie_not_first += int(len(tied) > 1 and best[s] != tied.min())
        self.stages += 1
        self.stages_nothing_kept += int(not keep.any() and act.any())
        self.stages_all_inactive += int(not act.any())

    def check(self):
        """The generator's own conditions."""
        assert min(self.alone.values()) >= 20, self.alone
        assert min(self.decided.values()) >= 1, self.decided
        assert self.tie_not_first >= 50, self.tie_not_first
        assert self.threshold_only >= 50, self.threshold_only
        assert self.stages_nothing_kept >= 1 and self.stages_all_inactive >= 1, (self.stages_nothing_kept, self.stages_all_inactive)

    def __repr__(self):
        return (f"{self.stages} stages: reject alone {self.alone}, rows decided by a NaN rule {self.decided}, by the tie-break "
                f"(winner not first) {self.tie_not_first}, by thres_error alone {self.threshold_only}; nothing kept in "
                f"{self.stages_nothing_kept} stages, all inactive in {self.stages_all_inactive}")

"""CPU-only: object tracks across the files of a log (include/icpflow_hip.h 8(l): icpflow_rows_carry, icpflow_pair_row_ids,
icpflow_object_tracks_extend_side, icpflow_object_tracks_path; csrc/carry.hip, csrc/tracks.hip).  The numpy restatement
(tests/carry_restatement.py) is held against plain loops and hand values, the pose chain against np.linalg.inv, and the entry
points refuse bad arguments with their codes and messages before any launch -- no GPU is needed for a refusal."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carry_cases as cc                      # noqa: E402
import carry_restatement as cr                # noqa: E402
import track_cases as tc                      # noqa: E402
import track_restatement as trk               # noqa: E402

F = np.float32
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
NEW = ("icpflow_rows_carry", "icpflow_rows_carry_workspace_bytes", "icpflow_pair_row_ids", "icpflow_pair_row_ids_workspace_bytes",
       "icpflow_object_tracks_extend_side", "icpflow_object_tracks_path", "icpflow_object_tracks_path_default_params")


def test_the_library_is_built_from_carry_hip_and_keeps_its_number():
    from icp_flow_amd import _lib, build, utils_tracks
    assert "carry.hip" in build.SOURCES
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "icpflow_hip.h")).read()
    for name in NEW:
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(_lib._L, name)
    assert "8(l)  object tracks across the files of a log" in hdr and _lib.VERSION == 215
    assert (_lib.CARRY_COUNTS, _lib.PAIR_ROW_ID_COUNTS, _lib.PAIR_ROW_ID_MAX_PAIRS, _lib.TRACK_PATH_COLS, _lib.TRACK_PATH_COUNTS) == (
        cr.CARRY_COUNTS, cr.ROW_ID_COUNTS, cr.MAX_PAIRS, cr.PATH_COLS, cr.PATH_COUNTS)
    for define, value in (("ICPFLOW_CARRY_COUNTS", 6), ("ICPFLOW_PAIR_ROW_ID_COUNTS", 3), ("ICPFLOW_PAIR_ROW_ID_MAX_PAIRS", 4096),
                          ("ICPFLOW_TRACK_PATH_COLS", 24), ("ICPFLOW_TRACK_PATH_COUNTS", 5)):
        assert f"#define {define} {value}\n" in hdr
    p = _lib.TrackPathParams.defaults()
    assert ctypes.sizeof(_lib.TrackPathParams) == 24 and (p.struct_size, p.max_dv, p.min_speed) == (24, cr.MAX_DV, cr.MIN_SPEED) == (24, 1.0, 0.5)
    assert (utils_tracks.CARRY_RADIUS, utils_tracks.CARRY_MIN_SHARE, utils_tracks.MAX_DV) == (cr.CARRY_RADIUS, cr.CARRY_MIN_SHARE, cr.MAX_DV) == (0.02, 0.5, 1.0)
    with pytest.raises(TypeError):
        _lib.TrackPathParams.defaults(struct_size=1)


# ------------------------------------------------------------------------------------------------------------------- the carry

def _brute_carry(prev, prev_id, pose, nxt, radius, min_share):
    """every pair of rows in a double loop of float32 scalar operations, the minimum kept with `<` (the lowest row on a tie)"""
    M = np.asarray(pose, np.float64).astype(F)
    rf = F(radius)
    r2, far = rf * rf, F(1e6)
    good = lambda p: all(abs(v) <= far for v in p)     # noqa: E731  (a NaN fails)
    moved = []
    for p in prev:
        q = [((M[r, 0] * p[0] + M[r, 1] * p[1]) + M[r, 2] * p[2]) + M[r, 3] for r in range(3)]
        moved.append(q if good(p) and good(q) else None)
    ids, d2s, idxs, counts = [], [], [], [0] * 6
    counts[4] = sum(q is None for q in moved)
    for x in nxt:
        if not good(x):
            ids.append(-1), d2s.append(r2), idxs.append(-2)
            counts[3] += 1
            continue
        best, at = None, -1
        for j, t in enumerate(moved):
            if t is None:
                continue
            dx, dy, dz = x[0] - t[0], x[1] - t[1], x[2] - t[2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= r2 and (best is None or d2 < best):
                best, at = d2, j
        idxs.append(at), d2s.append(r2 if at < 0 else best)
        ids.append(int(prev_id[at]) if at >= 0 and prev_id[at] >= 0 else -1)
        counts[0] += at >= 0
        counts[1] += ids[-1] >= 0
        counts[2] += at < 0
    if float(counts[0]) < min_share * float(len(nxt)):
        counts[5], ids = 1, [-1] * len(nxt)
    return np.array(ids, np.int32), np.array(d2s, F), np.array(idxs, np.int32), np.array(counts, np.int64)


def test_the_carry_equals_a_brute_force_minimum_on_200_seeded_view_pairs():
    rng = np.random.default_rng(2026)
    poses = list(cc.POSES.values())
    with np.errstate(all="ignore"):
        for k in range(200):
            n, m = int(rng.integers(0, 25)), int(rng.integers(0, 25))
            pose = poses[k % 3]
            prev, prev_id, nxt = cc.views(n, m, 1000 + k, pose)
            if k % 5 == 0 and m > 2:                        # duplicates, a NaN, a pad row
                prev[1] = prev[0]
                prev[2] = [np.nan, 0, 0] if k % 2 else [1e8, 1e8, 1e8]
            if k % 7 == 0 and n > 1:
                nxt[0] = [0, np.inf, 0]
            share = (0.0, 0.5, 1.0)[k % 3]
            got = cr.rows_carry(prev, prev_id, pose, nxt, cc.RADIUS, share)
            ids, d2, idx, counts = _brute_carry(prev, prev_id, pose, nxt, cc.RADIUS, share)
            assert np.array_equal(got["id"], ids) and np.array_equal(got["idx"], idx) and np.array_equal(got["counts"], counts), k
            assert np.array_equal(got["d2"].view(np.int32), d2.view(np.int32)), k


def test_the_views_hit_miss_and_break_as_their_text_claims():
    prev, prev_id, nxt = cc.views(513, 513, 3, cc.POSES["yaw30"])
    got = cr.rows_carry(prev, prev_id, cc.POSES["yaw30"], nxt, cc.RADIUS, 0.5)
    assert 0.6 * 513 < got["counts"][0] < 513 and got["counts"][2] > 20 and got["counts"][5] == 0 and 0 < got["counts"][1] < got["counts"][0]
    off = cc.rigid(30.0, (5.0, -3.0 + 5.0, 0.2))                 # 5 m off: nothing meets, the chain breaks
    broken = cr.rows_carry(prev, prev_id, off, nxt, cc.RADIUS, 0.5)
    assert broken["counts"][0] < 10 and broken["counts"][5] == 1 and (broken["id"] == -1).all()
    hit, miss = cc.at_radius()
    r2 = F(cc.RADIUS) * F(cc.RADIUS)
    assert hit * hit <= r2 < miss * miss and miss == np.nextafter(hit, F(np.inf))
    got = cr.rows_carry([[0, 0, 0]], [7], np.eye(4), [[hit, 0, 0], [miss, 0, 0]], cc.RADIUS, 0.0)
    assert got["id"].tolist() == [7, -1] and got["idx"].tolist() == [0, -1]
    # a pad row stays bad under the rotation that cancels it: (x - y) / sqrt 2 is small, the row itself is not
    got = cr.rows_carry([[1e8, 1e8, 1e8]], [3], cc.rigid(45.0), [[0, 0, 0]], 1000.0, 0.0)
    assert got["counts"].tolist() == [0, 0, 1, 0, 1, 0]


# ----------------------------------------------------------------------------------------------------------------- the pair ids

def _loop_row_ids(labels, rows, col, ids, weight):
    """a dictionary filled pair by pair: key -> (weight, id) of the pair that wins so far"""
    table, shared, seen = {}, 0, set()
    for p in range(len(ids)):
        k = cr.br.label_key(rows[p, col])
        shared += k in seen
        seen.add(k)
        if ids[p] < 0:
            continue
        w = 0.0 if weight is None else float(weight[p])
        w = -math.inf if w != w else w
        if k not in table or w > table[k][0]:
            table[k] = (w, int(ids[p]))
    out = [table.get(cr.br.label_key(v), (0, -1))[1] if not (v < 0) else -1 for v in labels]
    return np.array(out, np.int32), shared


def test_the_row_ids_equal_a_dictionary_loop():
    rng = np.random.default_rng(5)
    with np.errstate(invalid="ignore"):
        for k in range(60):
            P = int(rng.integers(0, 80))
            pool, rows, ids, weight = cc.pair_table(P, 300 + k, labels=12)
            labels = pool[rng.integers(0, len(pool), 200)]
            for col in (0, 1):
                for w in (None, weight):
                    got, counts = cr.pair_row_ids(labels, rows, col, ids, w)
                    want, shared = _loop_row_ids(labels, rows, col, ids, w)
                    assert np.array_equal(got, want) and counts.tolist() == [(want >= 0).sum(), (want < 0).sum(), shared], (k, col)
    rows = np.array([[1, 5], [2, 5], [3, 5], [4, -0.0], [5, cc.NAN_A]], F)
    labels = np.array([5, 0.0, -0.0, cc.NAN_A, cc.NAN_B, -1, 6], F)
    assert cr.pair_row_ids(labels, rows, 1, [10, 11, 12, 13, 14], [1.0, 3.0, 2.0, 0, 0])[0].tolist() == [11, 13, 13, 14, -1, -1, -1]
    assert cr.pair_row_ids(labels, rows, 1, [10, 11, 12, 13, 14], [3.0, 3.0, 3.0, 0, 0])[0].tolist()[0] == 10        # a tie: the lowest p
    assert cr.pair_row_ids(labels, rows, 1, [-1, 11, 12, 13, 14], None)[0].tolist()[0] == 11                         # ids -1 never win
    assert cr.pair_row_ids(labels, rows, 1, [-1, -1, -1, 13, 14], None)[0].tolist()[0] == -1
    assert cr.pair_row_ids(labels, rows, 1, [10, 11, 12, 13, 14], [np.nan, 1.0, np.nan, 0, 0])[0].tolist()[0] == 11   # a NaN weighs least
    assert cr.pair_row_ids(labels, rows, 1, [10, 11, 12, 13, 14], None)[1].tolist() == [4, 3, 2]


def test_side_0_is_side_1_with_the_label_columns_exchanged():
    step = tc.chain()[0]
    objects = np.array([tc.object_row(label_dst=999.0, label_src=10.0), tc.object_row(label_dst=20.0, label_src=999.0)])
    state = np.full(tc.CHAIN_ROWS, -1, np.int32)
    one, zero = cr.extend_side(step["labels"], state, 0, objects, 1, 1, 0.1), cr.extend_side(step["labels"], state, 0, objects, 0, 1, 0.1)
    assert one["obs"][:, 0].tolist() == [-1, 1] and zero["obs"][:, 0].tolist() == [0, -1]
    assert np.array_equal(one["track_of_row"], zero["track_of_row"]) and np.array_equal(one["segments"], zero["segments"])


# -------------------------------------------------------------------------------------------------------------------- the paths

def test_the_three_step_chain_gives_its_hand_values():
    obs, step, frames, want = cc.three_step_chain()
    paths, counts = cr.path(obs, step, frames, 2)
    assert paths[0].tolist() == [float(v) for v in want] and paths[1].tolist() == [1.0] + [0.0] * 23 and counts.tolist() == [2, 1, 1, 0, 1]
    smooth, counts = cr.path(obs, step, frames, 1, max_dv=2.0)                 # `<=`: exactly max_dv is smooth
    assert smooth[0, 16] == 1 and counts.tolist() == [1, 1, 1, 1, 1]
    gap, _ = cr.path([obs[0], obs[2]], [0, 2], frames, 1)                     # a missing step: no adjacent pair, not judged
    assert gap[0, 1:5].tolist() == [2, 0, 2, 1] and gap[0, 11:17].tolist() == [0, 0, 0, 1, 0, 0]
    two, _ = cr.path([obs[0], obs[1], obs[2]], [0, 0, 1], frames, 1)          # two in step 0: the one with more points counts
    assert two[0, 1] == 2 and two[0, 21:24].tolist() == [1.25, 2.0, 0.5] and two[0, 12] == 1 and two[0, 11] == 2.0
    tie, _ = cr.path([obs[0], obs[0][:10] + [9.0, 9.0, 9.0]], [0, 0], frames, 1)      # equal points: the lower row
    assert tie[0, 21:24].tolist() == [1.0, 2.0, 0.5]
    out, counts = cr.path(obs, [0, 1, 3], frames, 1)                          # a step outside [0, F): not counted
    assert out[0, 1] == 2 and out[0, 3] == 1 and counts.tolist() == [1, 1, 1, 1, 1]
    assert cr.path(np.zeros((0, 13)), [], np.zeros((0, 12)), 0)[1].tolist() == [0] * 5


def test_the_path_table_equals_a_vectorised_computation():
    """Per track and step the counted observation by a lexsort, the sums by numpy: the same numbers up to the order of the sums
    -- at most 5 terms of a few metres: 1e-12 is 10^3 roundings of such a sum."""
    for seed in range(40):
        obs, step, frames, T = cc.random_path_table(seed)
        paths, counts = cr.path(obs, step, frames, T)
        for t in range(T):
            rows = [k for k in range(len(obs)) if obs[k, 0] == t and 0 <= step[k] < len(frames)]
            best = {}
            for k in rows:
                if step[k] not in best or obs[k, 9] > obs[best[step[k]], 9]:
                    best[int(step[k])] = k
            steps = sorted(best)
            assert paths[t, 1] == len(steps)
            if not steps:
                assert not paths[t, 1:].any()
                continue
            R = [frames[s, :9].reshape(3, 3) for s in steps]
            d = np.array([R[i] @ obs[best[s], 3:6] for i, s in enumerate(steps)])
            c = np.array([R[i] @ obs[best[s], 10:13] + frames[s, 9:] for i, s in enumerate(steps)])
            v = d / obs[[best[s] for s in steps], 2][:, None]
            adj = [i for i in range(len(steps) - 1) if steps[i + 1] == steps[i] + 1]
            want_dv = max([np.hypot(*(v[i + 1] - v[i])[:2]) for i in adj], default=0.0)
            want_jump = max([np.hypot(*(c[i] + d[i] - c[i + 1])[:2]) for i in adj], default=0.0)
            secs = obs[[best[s] for s in steps], 2].sum()
            want = [len(steps), steps[0], steps[-1], steps[-1] - steps[0] + 1 - len(steps), secs, np.hypot(d[:, 0], d[:, 1]).sum(), *(d.sum(axis=0) / secs)]
            assert np.allclose(paths[t, 1:10], want, rtol=0, atol=1e-12), (seed, t)
            assert abs(paths[t, 11] - want_dv) <= 1e-12 and paths[t, 12] == len(adj) and abs(paths[t, 13] - want_jump) <= 1e-10, (seed, t)
            assert np.allclose(paths[t, 21:24], c[0], rtol=0, atol=1e-12) and paths[t, 20] == max(obs[best[s], 9] for s in steps)
        assert counts[0] == T and counts[1] == (paths[:, 1] > 0).sum() and counts[2] == (paths[:, 12] > 0).sum()


def test_the_pose_chain_equals_numpys_inverse():
    rng = np.random.default_rng(9)
    poses = [cc.rigid(rng.uniform(-180, 180), rng.normal(0, 3, 3), rng.uniform(-3, 3)) for _ in range(12)]
    frames = cr.frames_chain(poses)
    W = np.eye(4)
    for k, pose in enumerate(poses):
        if k:
            W = W @ np.linalg.inv(pose)
        assert np.abs(frames[k, :9].reshape(3, 3) - W[:3, :3]).max() <= 1e-12 and np.abs(frames[k, 9:] - W[:3, 3]).max() <= 1e-12
    assert frames[0].tolist() == cc.IDENTITY_FRAME
    from icp_flow_amd import pair_judges
    assert np.array_equal(pair_judges.log_frames(poses), frames)


# -------------------------------------------------------------------------------------------------------------------------- ABI

def _lib_and_fakes():
    from icp_flow_amd import _lib
    return _lib, _lib._L, ctypes.c_void_p(4096)


def test_the_carry_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    eye = np.eye(4).reshape(16)

    def call(**over):
        a = dict(prev=one, prev_id=one, m=100, pose=eye, next=one, n=90, radius=0.02, share=0.5, id=one, d2=None, idx=None, counts=one, ws=one,
                 ws_bytes=1 << 30)
        a.update(over)
        pose = None if a["pose"] is None else np.ascontiguousarray(a["pose"], np.float64).ctypes.data_as(ctypes.c_void_p)
        rc = L.icpflow_rows_carry(a["prev"], a["prev_id"], a["m"], pose, a["next"], a["n"], a["radius"], a["share"], a["id"], a["d2"], a["idx"],
                                  a["counts"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
        return rc, L.icpflow_last_error().decode()

    def pose_with(k, v):
        p = eye.copy()
        p[k] = v
        return p

    need = int(L.icpflow_rows_carry_workspace_bytes(90, 100))
    cases = [(dict(n=-1), E_ARG, "negative"), (dict(m=-1), E_ARG, "negative"), (dict(n=(1 << 29) + 1), E_LIMIT, "at most"),
             (dict(m=(1 << 29) + 1), E_LIMIT, "at most"), (dict(radius=0.0009), E_ARG, "radius"), (dict(radius=1001.0), E_ARG, "radius"),
             (dict(radius=float("nan")), E_ARG, "radius"), (dict(share=-0.1), E_ARG, "min_share"), (dict(share=1.5), E_ARG, "min_share"),
             (dict(share=float("nan")), E_ARG, "min_share"), (dict(pose=pose_with(3, np.nan)), E_ARG, "pose[3]"),
             (dict(pose=pose_with(15, np.inf)), E_ARG, "pose[15]"), (dict(pose=pose_with(0, 1e300)), E_ARG, "pose[0]"),
             (dict(ws=None), E_WORKSPACE, "icpflow_rows_carry_workspace_bytes"), (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"),
             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("prev", "prev_id", "pose", "next", "id", "counts")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_rows_carry"), (over, rc, msg)


def test_the_row_ids_refuse_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()

    def call(**over):
        a = dict(labels=one, n=100, pairs=one, P=5, stride=10, col=1, pid=one, weight=one, wstride=24, out=one, counts=one, ws=one, ws_bytes=1 << 30)
        a.update(over)
        rc = L.icpflow_pair_row_ids(a["labels"], a["n"], a["pairs"], a["P"], a["stride"], a["col"], a["pid"], a["weight"], a["wstride"], a["out"],
                                    a["counts"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
        return rc, L.icpflow_last_error().decode()

    need = int(L.icpflow_pair_row_ids_workspace_bytes(5))
    cases = [(dict(n=-1), E_ARG, "negative"), (dict(P=-1), E_ARG, "negative"), (dict(n=(1 << 29) + 1), E_LIMIT, "at most"),
             (dict(P=4097), E_LIMIT, "at most 4096"), (dict(col=2), E_ARG, "col"), (dict(col=-1), E_ARG, "col"), (dict(stride=1), E_ARG, "pair_stride"),
             (dict(wstride=0), E_ARG, "weight_stride"), (dict(ws=None), E_WORKSPACE, "icpflow_pair_row_ids_workspace_bytes"),
             (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"), (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("labels", "pairs", "pid", "out", "counts")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_pair_row_ids"), (over, rc, msg)


def test_extend_side_refuses_what_extend_refuses_and_a_bad_side():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackParams.defaults()

    def call(**over):
        a = dict(labels=one, n=100, Lmax=16, state=one, next_id=one, objects=one, P=3, side=0, gap=1, seconds=0.1, params=good, segments=one, num=one,
                 obs=one, counts=one, ws=one, ws_bytes=1 << 30)
        a.update(over)
        rc = L.icpflow_object_tracks_extend_side(a["labels"], a["n"], a["Lmax"], a["state"], a["next_id"], a["objects"], a["P"], a["side"], a["gap"],
                                                 a["seconds"], ctypes.byref(a["params"]) if a["params"] is not None else None, a["segments"],
                                                 a["num"], a["obs"], a["counts"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
        return rc, L.icpflow_last_error().decode()

    need = int(L.icpflow_object_tracks_extend_workspace_bytes(100, 16))
    cases = [(dict(side=2), E_ARG, "side"), (dict(side=-1), E_ARG, "side"), (dict(n=-1), E_ARG, "negative"), (dict(P=-1), E_ARG, "negative"),
             (dict(n=(1 << 29) + 1), E_LIMIT, "at most"), (dict(Lmax=0), E_ARG, "Lmax"), (dict(Lmax=4097), E_LIMIT, "at most 4096"),
             (dict(gap=64), E_ARG, "gap"), (dict(seconds=0.0), E_ARG, "seconds"), (dict(params=None), E_ARG, "null pointer"),
             (dict(params=_lib.TrackParams.defaults(min_iou=0.0)), E_ARG, "min_iou"),
             (dict(ws=None), E_WORKSPACE, "icpflow_object_tracks_extend_workspace_bytes"), (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"),
             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("labels", "state", "next_id", "objects", "segments", "num", "obs", "counts")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_object_tracks_extend_side:"), (over, rc, msg)


def test_the_path_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackPathParams.defaults()

    def call(**over):
        a = dict(obs=one, step=one, M=5, frames=one, F=2, T=3, params=good, paths=one, counts=one)
        a.update(over)
        rc = L.icpflow_object_tracks_path(a["obs"], a["step"], a["M"], a["frames"], a["F"], a["T"],
                                          ctypes.byref(a["params"]) if a["params"] is not None else None, a["paths"], a["counts"], None)
        return rc, L.icpflow_last_error().decode()

    short = _lib.TrackPathParams.defaults()
    short.struct_size = 16
    cases = [(dict(M=-1), E_ARG, "negative"), (dict(T=-1), E_ARG, "negative"), (dict(F=-1), E_ARG, "negative"), (dict(F=0), E_ARG, "F = 0"),
             (dict(M=(1 << 24) + 1), E_LIMIT, "at most"), (dict(T=(1 << 24) + 1), E_LIMIT, "at most"), (dict(F=(1 << 24) + 1), E_LIMIT, "at most"),
             (dict(params=None), E_ARG, "null pointer"), (dict(params=short), E_ARG, "struct_size"),
             (dict(params=_lib.TrackPathParams.defaults(max_dv=-1.0)), E_ARG, "max_dv"),
             (dict(params=_lib.TrackPathParams.defaults(max_dv=float("inf"))), E_ARG, "max_dv"),
             (dict(params=_lib.TrackPathParams.defaults(min_speed=float("nan"))), E_ARG, "min_speed")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("obs", "step", "frames", "paths", "counts")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_object_tracks_path"), (over, rc, msg)
    assert L.icpflow_object_tracks_path_default_params(None) == E_ARG


def test_the_workspace_queries_are_aligned_and_never_shrink():
    _lib, L, _ = _lib_and_fakes()
    ns = [0, 1, 2, 63, 512, 513, 1024, 1025, 2049, 4097, 78000, 1 << 20, 1 << 29]
    fn = L.icpflow_rows_carry_workspace_bytes
    for m in ns:
        sizes = [int(fn(n, m)) for n in ns]
        assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes), (m, sizes)
        sizes = [int(fn(m, n)) for n in ns]
        assert sizes == sorted(sizes), (m, sizes)
    assert fn(-1, 5) == 0 and fn(5, -1) == 0 and fn((1 << 29) + 1, 5) == 0 and fn(5, (1 << 29) + 1) == 0
    assert fn(1000, 2000) < L.icpflow_nn_residual_workspace_bytes(1000, 2000, 1, 0)       # the same grids, no table
    sizes = [int(L.icpflow_pair_row_ids_workspace_bytes(P)) for P in (0, 1, 1024, 4096)]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    assert L.icpflow_pair_row_ids_workspace_bytes(-1) == 0 and L.icpflow_pair_row_ids_workspace_bytes(4097) == 0


def test_the_python_layer_has_no_cpu_path():
    import torch
    from icp_flow_amd import utils_tracks
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.rows_carry_device(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), np.eye(4), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.pair_row_ids_device(torch.zeros(4), torch.zeros(2, 10), 1, torch.zeros(2, dtype=torch.int32))


# --------------------------------------------------------------------------------------------------------------------- the log

def test_make_log_is_what_it_claims():
    """under the oracle's CPU DBSCAN with LOG_CLUSTER every object is exactly one cluster in every file, on both sides, the
    braking box too, and nothing merges; every shared view pair has 0.70 to 0.90 of its rows with a partner within CARRY_RADIUS,
    each partner the same object; no two rows of different objects (the ground is one) lie within 10 x the radius"""
    from types import SimpleNamespace
    from icp_flow_amd import synthetic as sy
    from oracle import cluster as oc
    pairs, truth = sy.make_log(0, 6)
    a = SimpleNamespace(epsilon=sy.LOG_CLUSTER["epsilon"], min_cluster_size=sy.LOG_CLUSTER["min_cluster_size"], num_clusters=sy.LOG_CLUSTER["num_clusters"])
    objects = len(sy.LOG_SIZES)
    assert len(pairs) == 6 and truth["velocity"].shape == (objects, 6, 3) and truth["seen"].shape == (objects, 6)
    for k, pair in enumerate(pairs):
        pts = np.concatenate([pair["points_dst"], pair["points_src"]]).astype(np.float64)       # dst first, as cluster_frame_pair stacks them
        ids = np.concatenate([truth["ids_dst"][k], truth["ids_src"][k]])
        assert np.array_equal(ids != -1, np.concatenate([pair["nonground_dst"], pair["nonground_src"]]))
        labels = oc.cluster_pcd(a, pts, ids != -1)
        assert (labels[ids == -2] == -1).all() and (ids == -2).sum() >= 8                  # the isolated points are noise
        seen = {}
        for j in range(objects):
            mine = set(labels[ids == j].tolist())
            assert truth["seen"][j, k] == bool((truth["ids_src"][k] == j).any())     # seen: in the SOURCE sweep of the file
            if not truth["seen"][j, k]:
                assert j == sy.LOG_LATE and k < sy.LOG_LATE_FILE
                if not mine:                                                        # (file LOG_LATE_FILE - 1 has it in its destination)
                    continue
            assert len(mine) == 1 and min(mine) >= 0, (k, j, mine)           # one cluster over both sides, no noise in it
            seen[j] = mine.pop()
        assert len(set(seen.values())) == len(seen), (k, seen)               # nothing merges
        for side in ("src", "dst"):                                          # rows of different objects keep their distance
            p, o = pair["points_" + side].astype(np.float64), truth["ids_" + side][k]
            assert p[o >= 0, 2].min() - p[o == -1, 2].max() > 10 * cr.CARRY_RADIUS       # the ground lies below every object
            above = p[o != -1]
            box = np.array([above[o[o != -1] == j].mean(axis=0) if (o == j).any() else np.full(3, np.nan) for j in range(objects)])
            for j in range(objects):                                         # (only objects within 12 m of one another are compared row by row)
                for i in range(j):
                    if not ((o == i).any() and (o == j).any()):
                        continue
                    if np.linalg.norm(box[i] - box[j]) < 12.0:
                        d2 = ((p[o == i][:, None, :] - p[o == j][None, :, :]) ** 2).sum(axis=2)
                        assert d2.min() > (10 * cr.CARRY_RADIUS) ** 2, (k, side, i, j)
                    else:
                        reach = [np.linalg.norm(p[o == q] - box[q], axis=1).max() for q in (i, j)]
                        assert not (np.linalg.norm(box[i] - box[j]) - sum(reach) <= 10 * cr.CARRY_RADIUS), (k, side, i, j)
            lonely = p[o == -2]
            assert all(np.linalg.norm(p[o >= 0] - q, axis=1).min() > 1.0 for q in lonely)
    for k in range(1, 6):
        got = cr.rows_carry(pairs[k - 1]["points_dst"], truth["ids_dst"][k - 1], pairs[k]["pose"], pairs[k]["points_src"], cr.CARRY_RADIUS, cr.CARRY_MIN_SHARE)
        share = got["counts"][0] / len(pairs[k]["points_src"])
        assert 0.70 <= share <= 0.90 and got["counts"][5] == 0, (k, share)
        hit = got["idx"] >= 0
        assert np.array_equal(got["id"][hit], np.maximum(truth["ids_src"][k], -1)[hit])   # a partner is the same surface sample: the same object
    v = np.linalg.norm(truth["velocity"][sy.LOG_BRAKING], axis=1)
    assert np.allclose(v[: sy.LOG_BRAKE_FILE], 5.0) and np.allclose(v[sy.LOG_BRAKE_FILE:], 2.0)          # it loses 3 m/s between two files
    steady = [j for j in range(objects) if j != sy.LOG_BRAKING]
    assert np.abs(np.diff(truth["velocity"][steady], axis=1)).max() < 1e-12
    assert not truth["velocity"][sy.LOG_WALL].any() and truth["seen"][sy.LOG_LATE].tolist() == [False, False, True, True, True, True]
    assert any(not np.allclose(pair["pose"][:3, :3], np.eye(3)) for pair in pairs)                        # the ego vehicle turns


def test_the_command_line_knows_the_flags_and_refuses_what_is_not_built(tmp_path):
    from icp_flow_amd import frame_pairs, pair_judges
    ns = frame_pairs.argument_parser().parse_args(["dir"])
    assert (ns.tracks_log, ns.tracks_log_radius, ns.tracks_log_min_share, ns.tracks_log_max_dv) == (None, 0.02, 0.5, 1.0)
    ns = frame_pairs.argument_parser().parse_args(["dir", "--tracks-log", "--tracks-log-radius", "0.05", "--tracks-log-min-share", "0.3", "--tracks-log-max-dv", "2"])
    assert (ns.tracks_log, ns.tracks_log_radius, ns.tracks_log_min_share, ns.tracks_log_max_dv) == (True, 0.05, 0.3, 2.0)
    assert frame_pairs.argument_parser().parse_args(["dir", "--tracks-log", "out.jsonl"]).tracks_log == "out.jsonl"
    with pytest.raises(SystemExit, match="--tracks-log is not built into --protocol reference"):
        frame_pairs.main([str(tmp_path), "--tracks-log", "--protocol", "reference"])
    for flag, value in (("--tracks-log-radius", "0"), ("--tracks-log-min-share", "1.5"), ("--tracks-log-max-dv", "-1"), ("--sweep-seconds", "0")):
        with pytest.raises(SystemExit, match=flag):
            frame_pairs.main([str(tmp_path), "--tracks-log", flag, value])
    os.environ["WORLD_SIZE"] = "2"
    try:
        with pytest.raises(SystemExit, match="--tracks-log under more than one rank"):
            frame_pairs.main([str(tmp_path), "--tracks-log"])
    finally:
        del os.environ["WORLD_SIZE"]
    np.savez(str(tmp_path / "sample.npz"), **tc.scene()["arrays"])
    with pytest.raises(SystemExit, match="--tracks-log takes frame-pair files"):
        frame_pairs.main([str(tmp_path), "--tracks-log"])
    a = frame_pairs.default_args()
    a.tracks_log = True
    with pytest.raises(ValueError, match="args.tracks_log under more than one rank"):
        frame_pairs.run_stream(a, [], "cpu", rank=0, world=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        pair_judges.LogChain("cpu")


def test_log_tracks_reads_a_table_into_dicts_and_lines():
    from icp_flow_amd import utils_tracks
    obs, step, frames, _ = cc.three_step_chain()
    rows, counts = cr.path(obs, step, frames, 2)
    t = utils_tracks.LogTracks(rows[:1], counts, 1, [np.array([o]) for o in obs], [np.zeros(6), np.array([9, 7, 1, 0, 0, 0]), np.array([2, 0, 8, 0, 0, 1])],
                               [np.zeros(6)] * 3, frames, ["a", "b", "c"], [10, 10, 10], dict(max_dv=1.0))
    assert t.summary() == dict(files=3, tracks=1, observed=1, judged=1, smooth=0, rough=1, moving=1, breaks=1, carried_rows=7, rows=20, overflow=0)
    assert t.breaks() == [2]
    listed = t.as_list()
    assert len(listed) == 1 and listed[0]["track"] == 0 and listed[0]["counted"] == 3 and listed[0]["dv_max"] == 2.0 and not listed[0]["smooth"]
    assert [o["velocity"] for o in listed[0]["observations"]] == [[2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [4.0, 1.0, 0.0]]
    assert [(o["step"], o["file"], o["pair"]) for o in listed[0]["observations"]] == [(0, "a", 0), (1, "b", 0), (2, "c", 0)]
    assert len(utils_tracks.format_log_tracks(listed)) == 2

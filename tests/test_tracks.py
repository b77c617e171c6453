"""CPU-only: the object tracks (icpflow_label_overlap, icpflow_object_tracks_extend, icpflow_object_tracks_fit;
csrc/overlap.hip, csrc/tracks.hip; utils_tracks).  The numpy restatement (tests/track_restatement.py) is held against a dense
contingency matrix on seeded random labellings, every tie case is shown to be the tie its name claims, the hand-made chain and
the end-to-end scene are shown to be what they claim, the fit is held against np.linalg.lstsq, and the entry points refuse bad
arguments with their codes and messages before any launch -- no GPU is needed for a refusal."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as tc                      # noqa: E402
import track_restatement as trk               # noqa: E402

F = np.float32
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3


def test_the_library_is_built_from_the_track_sources_and_keeps_its_number():
    from icp_flow_amd import _lib, build
    assert {"overlap.hip", "tracks.hip"} <= set(build.SOURCES) and "overlap.hpp" in build.HEADERS
    hdr = open(os.path.join(os.path.dirname(build.HERE), "include", "icpflow_hip.h")).read()
    for name in ("icpflow_label_overlap", "icpflow_label_overlap_workspace_bytes", "icpflow_object_tracks_default_params",
                 "icpflow_object_tracks_extend", "icpflow_object_tracks_extend_workspace_bytes", "icpflow_object_tracks_fit"):
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(_lib._L, name)
    assert "8(k)  object tracks" in hdr and _lib.VERSION == 215
    assert (_lib.OVERLAP_COLS, _lib.OVERLAP_COUNTS, _lib.TRACK_SEGMENT_COLS, _lib.TRACK_OBS_COLS, _lib.TRACK_COLS, _lib.TRACK_EXTEND_COUNTS,
            _lib.TRACK_FIT_COUNTS) == (trk.OVERLAP_COLS, trk.OVERLAP_COUNTS, trk.SEGMENT_COLS, trk.OBS_COLS, trk.TRACK_COLS, 6, 5)
    for define, value in (("ICPFLOW_OVERLAP_COLS", 10), ("ICPFLOW_TRACK_SEGMENT_COLS", 6), ("ICPFLOW_TRACK_OBS_COLS", 13), ("ICPFLOW_TRACK_COLS", 16)):
        assert f"#define {define} {value}\n" in hdr
    p = _lib.TrackParams.defaults()
    assert ctypes.sizeof(_lib.TrackParams) == 32
    assert (p.struct_size, p.min_iou, p.max_residual, p.min_speed) == (32, trk.MIN_IOU, trk.MAX_RESIDUAL, trk.MIN_SPEED) == (32, 0.5, 0.2, 0.5)
    with pytest.raises(TypeError):
        _lib.TrackParams.defaults(struct_size=1)


# ------------------------------------------------------------------------------------------------- restatement against brute force

def _dense(a, b):
    """the contingency matrix of two labellings over their linkable labels, by a double loop, and everything read off it"""
    (ra, sa), (rb, sb) = trk.segments(a), trk.segments(b)
    M = np.zeros((len(ra), len(rb)), np.int64)
    for i in range(len(sa)):
        if trk.linkable(ra[sa[i], 0]) and trk.linkable(rb[sb[i], 0]):
            M[sa[i], sb[i]] += 1
    return ra, rb, M


def _partner(row):
    best = -1
    for e, v in enumerate(row):
        if v > 0 and (best < 0 or v > row[best]):      # strictly greater: a tie stays with the lower index
            best = e
    return best


def _check_against_dense(a, b):
    ta, tb, num_a, num_b, counts = trk.label_overlap(a, b)
    ra, rb, M = _dense(a, b)
    assert (num_a, num_b) == (len(ra), len(rb))
    for table, rows, other, mat in ((ta, ra, rb, M), (tb, rb, ra, M.T)):
        partners = [_partner(mat[c]) for c in range(len(rows))]
        back = [_partner(mat.T[e]) for e in range(len(other))]
        for c in range(len(rows)):
            p = partners[c]
            rest = sorted(np.delete(mat[c], p).tolist() if p >= 0 else [0])
            want = [rows[c, 0], rows[c, 1], mat[c].sum(), p] + ([other[p, 0], mat[c, p], rest[-1] if rest else 0, other[p, 1], float(back[p] == c),
                                                                   mat[c, p] / (rows[c, 1] + other[p, 1] - mat[c, p])] if p >= 0 else [0.0] * 6)
            assert table[c].tolist() == [float(v) for v in want], (c, table[c], want)
    assert counts.tolist() == [M.sum(), sum(ta[:, 8]), (M.sum(axis=1) > 0).sum(), (M.sum(axis=0) > 0).sum()]


def test_the_restatement_equals_a_dense_contingency_matrix_on_200_random_labellings():
    rng = np.random.default_rng(20260)
    for k in range(200):
        n = int(rng.integers(1, 120))
        pool = np.array([-1e8, -1.0, -0.0, 0.0, 1.0, 2.0, 3.5, 7.0, 9.0][: int(rng.integers(2, 10))], F)
        _check_against_dense(rng.choice(pool, n), rng.choice(pool[::-1], n))
    for a, b in (tc.tie_two_two(), tc.tie_mutual(), tc.all_negative_other_side(), tc.relabelled(), tc.long_segment(tc.LONG_CUTS[2])):
        _check_against_dense(a, b)


def test_tie_two_two_is_a_tie_and_the_lower_index_takes_it():
    a, b = tc.tie_two_two()
    ra, rb, M = _dense(a, b)
    assert ra[:, 0].tolist() == [3, 7] and rb[:, 0].tolist() == [1, 2] and M[1].tolist() == [2, 2]
    ta = trk.label_overlap(a, b)[0]
    assert (ta[1, 3], ta[1, 4], ta[1, 5], ta[1, 6]) == (0, 1.0, 2, 2)


def test_tie_mutual_is_four_ties_and_the_rule_decides_who_is_mutual():
    a, b = tc.tie_mutual()
    _, _, M = _dense(a, b)
    assert M.tolist() == [[1, 1], [1, 1]]
    ta, tb, _, _, counts = trk.label_overlap(a, b)
    assert ta[:, 3].tolist() == [0, 0] and tb[:, 3].tolist() == [0, 0] and ta[:, 8].tolist() == [1, 0] and tb[:, 8].tolist() == [1, 0]
    # ties to the HIGHER index would have made the other two mutual: the partner rule, not the data, decides
    assert [max(range(2), key=lambda e: (M[c, e], e)) for c in range(2)] == [1, 1]
    assert counts.tolist() == [4, 1, 2, 2]


def test_overflow_and_nothing():
    ta, tb, num_a, num_b, counts = trk.label_overlap(np.arange(9, dtype=F), np.zeros(9, F), Lmax=8)
    assert (num_a, num_b, len(ta), len(tb)) == (-9, 1, 0, 0) and not counts.any()
    assert trk.label_overlap([], [])[2:4] == (0, 0)


# --------------------------------------------------------------------------------------------------------------------- the chain

def test_the_chain_is_what_its_text_claims():
    state, next_id = np.full(tc.CHAIN_ROWS, -1, np.int32), 0
    steps = tc.chain()
    for gap, step in enumerate(steps, start=1):
        got = trk.extend(step["labels"], state, next_id, None, gap, 0.1 * gap)
        assert got["track_of_row"].tolist() == step["ids"].tolist() and got["next_id"] == step["next_id"]
        assert got["segments"][:, 2].tolist() == step["segment_ids"] and got["segments"][:, 3].tolist() == step["inherited"]
        state, next_id = got["track_of_row"], got["next_id"]
    ta = trk.label_overlap(steps[1]["labels"], trk.track_labels(steps[0]["ids"]))[0]
    by_label = {row[0]: row for row in ta}
    assert by_label[8.0][9] == 4 / 6 and by_label[8.0][8] == 1                       # the larger part of the split: mutual
    assert by_label[9.0][3] == by_label[8.0][3] and by_label[9.0][8] == 0            # the smaller part: same partner, not mutual
    assert (by_label[11.0][5], by_label[11.0][6], by_label[11.0][9]) == (4, 3, 4 / 7)   # the merge: 4 rows of D, 3 of C
    assert (steps[1]["labels"][19:22] == -1).all() and steps[1]["ids"][19:22].tolist() == [4, 4, 4]    # unseen, its rows keep the id
    tb = trk.label_overlap(steps[2]["labels"], trk.track_labels(steps[1]["ids"]))[0]
    assert tb[2].tolist() == [2.0, 3, 2, 5, 5.0, 2, 0, 3, 1, 0.5] and 2 / (3 + 3 - 2) == 0.5   # IoU exactly min_iou, no rounding
    above = trk.extend(steps[2]["labels"], steps[1]["ids"], 7, None, 3, 0.3, min_iou=np.nextafter(0.5, 1.0))
    assert above["segments"][:, 2].tolist() == [-1, 4, 7]


def test_fresh_ids_follow_the_label_order_not_the_row_order():
    labels = np.array([9, 9, 5, 5, 7, 7, -1], F)              # the rows meet 9 first, the ids go 5, 7, 9
    got = trk.extend(labels, np.full(7, -1, np.int32), 10, None, 1, 0.1)
    assert got["track_of_row"].tolist() == [12, 12, 10, 10, 11, 11, -1] and got["next_id"] == 13


# ----------------------------------------------------------------------------------------------------------------------- the fit

def test_the_fit_equals_least_squares_through_the_origin():
    """v = (sum s d) / (sum s s) per axis with K observations: the numerator carries at most K roundings of products and K - 1 of
    sums, relative to sum |s d|; the denominator likewise, relative to itself; the quotient one more: |v - v_exact| <=
    (2 K + 3) u sum|s d| / sum s s to first order, u = 2^-53.  np.linalg.lstsq (an SVD of one column, condition 1) is backward
    stable: its own error is a small multiple of u |d| / |s| >= u sum|s d| / sum s s (Cauchy-Schwarz); 16 u |d| / |s| is allowed
    for it."""
    rng = np.random.default_rng(5)
    u = 2.0 ** -53
    for K in (2, 3, 8):
        for _ in range(20):
            s = 0.1 * rng.integers(1, 16, K)
            v = rng.normal(0, 5, 3)
            d = s[:, None] * v + rng.normal(0, 0.05, (K, 3))
            obs = [tc.observation(0, g, s[g], d[g]) for g in range(K)]
            tracks, _ = trk.fit(obs, 1)
            want = np.linalg.lstsq(s[:, None], d, rcond=None)[0][0]
            for a in range(3):
                bound = (2 * K + 3) * u * np.abs(s * d[:, a]).sum() / (s * s).sum() + 16 * u * np.linalg.norm(d[:, a]) / np.linalg.norm(s)
                assert abs(tracks[0, 3 + a] - want[a]) <= bound, (K, a, tracks[0, 3 + a], want[a], bound)
            r = d[:, :2] - s[:, None] * tracks[0, 3:5]
            assert abs(tracks[0, 7] - np.sqrt((r * r).sum(axis=1).max())) <= 1e-12 and tracks[0, 6] == np.sqrt(tracks[0, 3] ** 2 + tracks[0, 4] ** 2)


def test_hand_made_motions():
    on = [tc.observation(1, g, 0.125 * g, (0.25 * g, -0.5 * g, 0.0625 * g)) for g in (1, 2)]
    tracks, counts = trk.fit(on + [tc.observation(-1, 1, 0.1, (5.0, 5.0, 5.0))], 2)
    assert tracks[1, :12].tolist() == [1, 2, 6, 2.0, -4.0, 0.5, np.sqrt(20.0), 0, 0, 1, 1, 1] and not tracks[0].any() and counts.tolist() == [2, 1, 1, 1, 1]
    one, _ = trk.fit(on[:1], 2)
    assert one[1, 9:12].tolist() == [1, 0, 0]                                 # one gap: not judged
    for side, consistent in ((-1, 1), (0, 1), (1, 0)):
        x = 0.2 if side == 0 else np.nextafter(0.2, side * np.inf)
        t, _ = trk.fit([tc.observation(0, 1, 0.5, (x, 0, 0)), tc.observation(0, 2, 0.5, (-x, 0, 0))], 1, max_residual=0.2)
        assert t[0, 3] == 0 and t[0, 7] == x and t[0, 10:12].tolist() == [1, consistent]
    sized, _ = trk.fit([tc.observation(0, 1, 0.1, (0, 0, 0), size=(4, 1, 2), points=7), tc.observation(0, 3, 0.3, (0, 0, 0), size=(3, 2, 1), points=9)], 1)
    assert sized[0, 12:16].tolist() == [4, 2, 2, 9] and sized[0, 2] == 10 and sized[0, 9] == 0


# --------------------------------------------------------------------------------------------------------------------- the scene

def test_the_scene_is_what_the_end_to_end_test_claims():
    """under the oracle's CPU DBSCAN with the test's parameters every object is exactly one cluster in every gap and nothing
    merges; on the true displacements the constant-velocity objects fit without residual and the bad one lies far beyond 0.2 m"""
    from oracle import cluster as oc
    sc = tc.scene()
    raw, t, obj = sc["arrays"]["raw_points"].astype(np.float64), sc["arrays"]["time_indice"], sc["object"]
    a = SimpleNamespace(epsilon=tc.SCENE_CLUSTER["epsilon"], min_cluster_size=tc.SCENE_CLUSTER["min_cluster_size"], num_clusters=tc.SCENE_CLUSTER["num_clusters"])
    for j in range(1, tc.SCENE_FRAMES):
        rows = np.concatenate([np.flatnonzero(t == 0), np.flatnonzero(t == j)])          # dst first, as cluster_frame_pair stacks them
        labels = oc.cluster_pcd(a, raw[rows], np.ones(len(rows), bool))
        dst = slice(0, int((t == 0).sum()))
        seen = {}
        for k in range(len(tc.SCENE_STEPS)):
            mine = set(labels[dst][obj[rows][dst] == k].tolist())
            assert len(mine) == 1 and min(mine) >= 0, (j, k, mine)                         # one cluster, no noise in it
            seen[k] = mine.pop()
        assert len(set(seen.values())) == len(seen)                                       # nothing merges
        assert (labels[obj[rows] == -1] == -1).all()
    S = tc.SCENE_SWEEP_SECONDS
    obs = []
    for k, step in enumerate(tc.SCENE_STEPS):
        for j in range(1, tc.SCENE_FRAMES):
            d = -(j * step + (tc.SCENE_BAD_OFFSET if (k == tc.SCENE_BAD and j == tc.SCENE_BAD_FRAME) else 0.0))
            obs.append(tc.observation(k, j, j * S, d))
    tracks, counts = trk.fit(obs, 5)
    good = [k for k in range(5) if k != tc.SCENE_BAD]
    assert (tracks[good, 7] < 1e-12).all() and np.allclose(tracks[good, 3:6], tc.scene_truth_velocity()[good], atol=1e-12)
    assert tracks[tc.SCENE_BAD, 7] > 0.2 + 0.2 and counts.tolist() == [5, 5, 5, 4, 4]     # far from the policy on both sides
    assert np.linalg.norm(tc.SCENE_BAD_OFFSET) == pytest.approx(1.0, abs=1e-3)
    assert (np.abs(tc.SCENE_STEPS).sum(axis=1) * 3 + 1.0 < 2.0 + 1.0).all()               # every displacement inside translation_frame


# --------------------------------------------------------------------------------------------------------------------------- ABI

def _lib_and_fakes():
    from icp_flow_amd import _lib
    return _lib, _lib._L, ctypes.c_void_p(4096)


def test_label_overlap_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()

    def call(**over):
        a = dict(a=one, b=one, n=100, Lmax=16, ta=one, na=one, tb=one, nb=one, counts=one, ws=one, ws_bytes=1 << 30)
        a.update(over)
        rc = L.icpflow_label_overlap(a["a"], a["b"], a["n"], a["Lmax"], a["ta"], a["na"], a["tb"], a["nb"], a["counts"], a["ws"],
                                     ctypes.c_size_t(a["ws_bytes"]), None)
        return rc, L.icpflow_last_error().decode()

    need = int(L.icpflow_label_overlap_workspace_bytes(100, 16))
    for over, code, text in ((dict(n=-1), E_ARG, "negative"), (dict(n=(1 << 29) + 1), E_LIMIT, "at most"), (dict(Lmax=0), E_ARG, "Lmax"),
                             (dict(Lmax=4097), E_LIMIT, "at most 4096"), (dict(a=None), E_ARG, "null pointer"), (dict(b=None), E_ARG, "null pointer"),
                             (dict(ta=None), E_ARG, "null pointer"), (dict(na=None), E_ARG, "null pointer"), (dict(tb=None), E_ARG, "null pointer"),
                             (dict(nb=None), E_ARG, "null pointer"), (dict(counts=None), E_ARG, "null pointer"),
                             (dict(ws=None), E_WORKSPACE, "icpflow_label_overlap_workspace_bytes"), (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"),
                             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")):
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_label_overlap"), (over, rc, msg)


def test_the_extension_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackParams.defaults()

    def call(**over):
        a = dict(labels=one, n=100, Lmax=16, state=one, next_id=one, objects=one, P=3, gap=1, seconds=0.1, params=good, segments=one, num=one,
                 obs=one, counts=one, ws=one, ws_bytes=1 << 30)
        a.update(over)
        rc = L.icpflow_object_tracks_extend(a["labels"], a["n"], a["Lmax"], a["state"], a["next_id"], a["objects"], a["P"], a["gap"], a["seconds"],
                                            ctypes.byref(a["params"]) if a["params"] is not None else None, a["segments"], a["num"], a["obs"],
                                            a["counts"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
        return rc, L.icpflow_last_error().decode()

    short = _lib.TrackParams.defaults()
    short.struct_size = 24
    need = int(L.icpflow_object_tracks_extend_workspace_bytes(100, 16))
    cases = [(dict(n=-1), E_ARG, "negative"), (dict(P=-1), E_ARG, "negative"), (dict(n=(1 << 29) + 1), E_LIMIT, "at most"), (dict(Lmax=0), E_ARG, "Lmax"),
             (dict(Lmax=4097), E_LIMIT, "at most 4096"), (dict(gap=-1), E_ARG, "gap"), (dict(gap=64), E_ARG, "gap"), (dict(seconds=0.0), E_ARG, "seconds"),
             (dict(seconds=float("inf")), E_ARG, "seconds"), (dict(seconds=float("nan")), E_ARG, "seconds"), (dict(params=None), E_ARG, "null pointer"),
             (dict(params=short), E_ARG, "struct_size"), (dict(params=_lib.TrackParams.defaults(min_iou=0.0)), E_ARG, "min_iou"),
             (dict(params=_lib.TrackParams.defaults(min_iou=1.5)), E_ARG, "min_iou"), (dict(params=_lib.TrackParams.defaults(min_iou=float("nan"))), E_ARG, "min_iou"),
             (dict(params=_lib.TrackParams.defaults(max_residual=-1.0)), E_ARG, "max_residual"),
             (dict(params=_lib.TrackParams.defaults(min_speed=float("inf"))), E_ARG, "min_speed"),
             (dict(ws=None), E_WORKSPACE, "icpflow_object_tracks_extend_workspace_bytes"), (dict(ws_bytes=need - 1), E_WORKSPACE, "workspace of"),
             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")]
    cases += [(dict(**{k: None}), E_ARG, "null pointer") for k in ("labels", "state", "next_id", "objects", "segments", "num", "obs", "counts")]
    for over, code, text in cases:
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_object_tracks_extend"), (over, rc, msg)
    assert L.icpflow_object_tracks_default_params(None) == E_ARG


def test_the_fit_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.TrackParams.defaults()

    def call(**over):
        a = dict(obs=one, M=5, T=3, params=good, tracks=one, counts=one)
        a.update(over)
        rc = L.icpflow_object_tracks_fit(a["obs"], a["M"], a["T"], ctypes.byref(a["params"]) if a["params"] is not None else None, a["tracks"], a["counts"], None)
        return rc, L.icpflow_last_error().decode()

    short = _lib.TrackParams.defaults()
    short.struct_size = 8
    for over, code, text in ((dict(M=-1), E_ARG, "negative"), (dict(T=-1), E_ARG, "negative"), (dict(M=(1 << 24) + 1), E_LIMIT, "at most"),
                             (dict(T=(1 << 24) + 1), E_LIMIT, "at most"), (dict(obs=None), E_ARG, "null pointer"), (dict(tracks=None), E_ARG, "null pointer"),
                             (dict(counts=None), E_ARG, "null pointer"), (dict(params=None), E_ARG, "null pointer"), (dict(params=short), E_ARG, "struct_size"),
                             (dict(params=_lib.TrackParams.defaults(max_residual=float("nan"))), E_ARG, "max_residual"),
                             (dict(params=_lib.TrackParams.defaults(min_speed=-0.5)), E_ARG, "min_speed")):
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_object_tracks_fit"), (over, rc, msg)


def test_the_workspace_queries_are_aligned_and_never_shrink():
    _lib, L, _ = _lib_and_fakes()
    ns = [0, 1, 2, 63, 1023, 1024, 1025, 4096, 4097, 63276, 126598, 1 << 20, 1 << 29]
    Ls = [1, 2, 16, 512, 4095, 4096]
    for fn in (L.icpflow_label_overlap_workspace_bytes, L.icpflow_object_tracks_extend_workspace_bytes):
        for Lmax in Ls:
            sizes = [int(fn(n, Lmax)) for n in ns]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes), (fn.__name__, Lmax, sizes)
        for n in ns:
            sizes = [int(fn(n, Lmax)) for Lmax in Ls]
            assert sizes == sorted(sizes), (fn.__name__, n, sizes)
        assert fn(-1, 16) == 0 and fn(10, 0) == 0 and fn(10, 4097) == 0 and fn((1 << 29) + 1, 16) == 0
    for n, Lmax in ((100, 16), (63276, 4096)):
        assert L.icpflow_object_tracks_extend_workspace_bytes(n, Lmax) > L.icpflow_label_overlap_workspace_bytes(n, Lmax)


# ------------------------------------------------------------------------------------------------------------------ Python layer

def test_tracks_reads_a_table_into_dicts_and_lines():
    from icp_flow_amd import utils_tracks
    obs = [tc.observation(1, g, 0.125 * g, (0.25 * g, -0.5 * g, 0.0), size=(4.0, 2.0, 1.5), points=40 + g) for g in (1, 2)]
    rows, counts = trk.fit(obs, 3)
    t = utils_tracks.Tracks(rows, counts, 3, [1, 2], [np.array([1]), np.array([1])], [np.array([2, 0, 2, 1, 0, 0]), np.array([2, 2, 0, 1, 0, 0])],
                            dict(min_iou=0.5, max_residual=0.2, min_speed=0.5))
    assert t.summary() == dict(tracks=3, observed=1, judged=1, consistent=1, inconsistent=0, moving=1, gaps=2, overflow=0)
    listed = t.as_list()
    assert len(listed) == 1 and listed[0] == dict(track=1, observations=2, gaps=[1, 2], velocity=[2.0, -4.0, 0.0], speed=np.sqrt(20.0), residual_max=0.0,
                                                  residual_rms=0.0, moving=True, judged=True, consistent=True, size=[4.0, 2.0, 1.5], points=42)
    assert len(utils_tracks.format_tracks(listed)) == 2
    import torch
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.label_overlap_device(torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_tracks.TrackState(4, "cpu")


def test_the_command_line_knows_the_flags_and_refuses_what_is_not_built():
    from icp_flow_amd import frame_pairs
    ns = frame_pairs.argument_parser().parse_args(["dir"])
    assert (ns.tracks, ns.tracks_min_iou, ns.tracks_max_residual) == (None, 0.5, 0.2)
    ns = frame_pairs.argument_parser().parse_args(["dir", "--tracks", "--tracks-min-iou", "0.6", "--tracks-max-residual", "0.3"])
    assert (ns.tracks, ns.tracks_min_iou, ns.tracks_max_residual) == (True, 0.6, 0.3)
    assert frame_pairs.argument_parser().parse_args(["dir", "--tracks", "out.jsonl"]).tracks == "out.jsonl"
    with pytest.raises(SystemExit, match="--tracks is not built into --protocol reference"):
        frame_pairs.main(["dir", "--tracks", "--protocol", "reference"])
    with pytest.raises(SystemExit, match="--tracks-min-iou"):
        frame_pairs.main(["dir", "--tracks", "--tracks-min-iou", "0"])
    a = frame_pairs.default_args()
    a.tracks = True
    with pytest.raises(ValueError, match="args.tracks under more than one rank"):
        frame_pairs.run_stream(a, [], "cpu", rank=0, world=2)


def test_load_sequence_tags_its_frame_pairs_and_the_samples_are_grouped(tmp_path):
    from icp_flow_amd import frame_pairs
    sc = tc.scene()
    path = str(tmp_path / "sample.npz")
    np.savez(path, **sc["arrays"])
    fps = frame_pairs.load_sequence(path)
    assert len(fps) == 3 and all(fp.sequence == path for fp in fps) and [fp.gap for fp in fps] == [1, 2, 3]
    assert all(np.array_equal(fp.points_dst, fps[0].points_dst) for fp in fps)
    lone = frame_pairs.FramePair(fps[0].points_src, fps[0].points_dst)
    assert lone.sequence is None
    sample_of, samples = {}, {}
    got = list(frame_pairs._by_sample([path, lone, lone] + fps[:2], None, sample_of, samples))
    assert len(got) == 7 and sample_of == {0: 0, 1: 0, 2: 0, 3: 1, 4: 2, 5: 3, 6: 3}
    assert [samples[s]["size"] for s in sorted(samples)] == [3, 1, 1, 2]
    short = frame_pairs.FramePair(fps[1].points_src, fps[1].points_dst[:-1], sequence=path)
    with pytest.raises(ValueError, match="disagree on the rows of the shared sweep"):
        list(frame_pairs._by_sample([fps[0], short], None, {}, {}))

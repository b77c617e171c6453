"""CPU-only: tests/match_eval_restatement.py against the oracle (oracle/reference_path.py: match_eval) on every case of
tests/match_eval_cases.py with two non-empty sides, its pre-selection against its plain form, and the conditions on the inputs of
tests/test_gpu_match_eval.py -- the path each case is built for and the geometry that makes it take that path's branches --
as conditions in numbers, not measurements."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import match_eval_cases as mc            # noqa: E402
import match_eval_restatement as mr      # noqa: E402
import sort_restatement as sr            # noqa: E402
from oracle import reference_path as rp  # noqa: E402

F = np.float32
NAMES = list(mc.CASES)


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", ["scan_q1_N257", "poses_N300", "threshold_scan_0.1", "threshold_sweep_0.5", "duplicates_scan_N1100", "sweep_rounds"])
def test_preselection_equals_the_plain_form(name):
    c = mc.get(name)
    recs, _ = mc.restated(name)
    for b, r in enumerate(recs):
        plain = mr.pair(c["P1"][b], c["P2"][b], c["T"][b], c["thres"], select=False)
        for d in range(2):
            assert np.array_equal(plain["d"][d].view(np.uint32), r["d"][d].view(np.uint32)), (name, b, d)


def test_empty_sides_by_the_contract():
    """a non-empty side against an empty one: +inf, no inliers; an empty query side: NaN (0 / 0), as the oracle gives"""
    _, out = mc.restated("empty_and_one_point_N300")
    assert out["errors"][0, 0] == np.inf and np.isnan(out["errors"][0, 1])          # (200, 0)
    assert np.isnan(out["errors"][1, 0]) and out["errors"][1, 1] == np.inf          # (0, 200)
    assert np.isnan(out["errors"][2]).all() and np.isnan(out["ratios"][2]).all()    # (0, 0)
    assert (out["inliers"][:3] == 0).all()
    assert out["ratios"][0, 0] == 0 and out["ious"][0, 0] == 0 and np.isnan(out["translations"][1]).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_oracle(name):
    """inliers, ratios, ious equal; errors at rtol 1e-5 and translations at 1e-5 of the two centroids they are the difference of --
    the oracle sums in float32 --; rotations at 1e-4 degrees.  Each pair at a width of its own (its longer cloud and one pad row:
    the oracle's search is un-lengthed, and a pad is never a valid row's neighbour while the other side has a row)."""
    c = mc.get(name)
    recs, out = mc.restated(name)
    args = SimpleNamespace(thres_dist=c["thres"])
    for b, r in enumerate(recs):
        if r["n1"] == 0 or r["n2"] == 0:
            continue
        W = min(c["P1"].shape[1], max(r["n1"], r["n2"]) + 1)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x[None]))      # noqa: E731
        with np.errstate(all="ignore"):
            o = [x[0].numpy() for x in rp.match_eval(args, t(c["P1"][b, :W]), t(c["P2"][b, :W]), t(c["T"][b]))]
        for k, got in zip(("inliers", "ratios", "ious"), o[1:4]):
            assert np.array_equal(got, out[k][b]), (name, b, k, got, out[k][b])
        assert np.allclose(o[0], out["errors"][b], rtol=1e-5, atol=0), (name, b, o[0], out["errors"][b])
        cm, co = np.abs(np.array(r["Sm"])) / r["n1"], np.abs(np.array(r["So"])) / r["n1"]
        assert (np.abs(o[4] - out["translations"][b]) <= 1e-5 * (cm + co) + 1e-12).all(), (name, b, o[4], out["translations"][b])
        assert np.allclose(o[5], out["rotations"][b], rtol=0, atol=1e-4, equal_nan=True), (name, b, o[5], out["rotations"][b])


def test_identity_rotation_prints_as_the_oracle():
    names, Ts = mc.rotation_poses()
    got = mr.rotations32(Ts[names.index("identity")])
    ref = rp.match_eval(SimpleNamespace(thres_dist=0.1), *[torch.from_numpy(mc.get("rotations_exact_N16")[k][:1]) for k in ("P1", "P2", "T")])[5][0].numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) and np.array_equal(np.signbit(got), [False, True, False])


# ------------------------------------------------------------------------------------------------ the paths
@pytest.mark.parametrize("name", NAMES)
def test_case_takes_the_path_it_is_built_for(name):
    c, spec = mc.get(name), mc.CASES[name]
    p = mc.paths(c)
    assert p["kernel"] == spec["kernel"], (name, p["kernel"])
    assert spec["has"] <= mc.tokens(p), (name, mc.tokens(p))
    B, N = c["P1"].shape[:2]
    again = mc.paths(c, no_eval_sweep=True)
    assert again["kernel"] == f"scan<{mc.scan_queries_per_lane(N, B)}>" and again["dirs"] is None
    for a in list(c["P1"]) + list(c["P2"]):      # the pad_segment layout: the flagged rows are a prefix, pads behind them
        n = mr.length(a)
        assert (a[:n, 3] == 1).all() and (a[n:] == sc_pad()).all()


def sc_pad():
    return np.array([1e8, 1e8, 1e8, 0.0], F)


def lens(c):
    return [(mr.length(a), mr.length(b)) for a, b in zip(c["P1"], c["P2"])]


def test_host_decisions_at_their_thresholds():
    assert not mc.eval_by_sweep(2, 2048) and mc.eval_by_sweep(1, 2049) and mc.eval_by_sweep(256, 1024) and not mc.eval_by_sweep(255, 1024)
    assert not mc.eval_by_sweep(1, 16385) and mc.eval_by_sweep(1, 16384) and not mc.eval_by_sweep(129, 1025)
    assert [mc.scan_queries_per_lane(n, b) for n, b in ((512, 999), (513, 1), (1024, 999), (1025, 128), (1025, 129))] == [1, 2, 2, 2, 4]
    assert not mc.share_instantiation(256, 1024) and mc.share_instantiation(128, 2048) and mc.share_scratch(128, 2048)
    # fullScan: at most two query blocks, at least 512 targets; sharedWindow: at most 64 rows in the last block, at least 512 targets
    assert mc.direction_path(512, 512, 1, 2049)[:2] == ("full", 4) and mc.direction_path(513, 512, 1, 2049)[0] == "shared"
    assert mc.direction_path(40, 511, 1, 2049)[0] == "window" and mc.direction_path(256, 512, 1, 2049)[:2] == ("full", 8)
    assert mc.direction_path(577, 2049, 1, 2049)[0] == "window" and mc.direction_path(576, 511, 1, 2049)[0] == "window"
    assert mc.direction_path(600, 4096, 1, 4112)[2] and not mc.direction_path(600, 4097, 1, 4112)[2]


# ------------------------------------------------------------------------------------------------ the geometry
def wave_view(c, rec, b, backward):
    """The sweep's waves of one direction of pair b: 64 consecutive queries of the sorted order -> list of dict(d: their distances,
    cu: their keys in the frame of the target keys, tk: the sorted target keys)"""
    p1, p2, M = c["P1"][b], c["P2"][b], c["T"][b]
    code, o1, o2 = mc.sorted_rows(p1, p2)
    if not backward:
        d, cu, tk = rec["d"][0][o1], sr.axis_key(code, rec["mv"][o1]), sr.axis_key(code, p2[o2, :3])
    else:
        raw = ((p2[o2, :3].astype(np.float64) - M[:3, 3].astype(np.float64)) @ M[:3, :3].astype(np.float64)).astype(F)     # R^T (c - t)
        d, cu, tk = rec["d"][1][o2], sr.axis_key(code, raw), sr.axis_key(code, p1[o1, :3])
    return [dict(d=d[i:i + 64], cu=cu[i:i + 64], tk=tk) for i in range(0, len(d), 64)]


def gap(w):
    """how far the nearest target key is from the wave's key range (0: inside it)"""
    lo, hi = w["cu"].min(), w["cu"].max()
    inside = (w["tk"] >= lo) & (w["tk"] <= hi)
    return 0.0 if inside.any() else float(np.minimum(np.abs(w["tk"] - lo), np.abs(w["tk"] - hi)).min())


def test_rounds_case_by_numbers():
    c = mc.get("sweep_rounds")
    recs, _ = mc.restated("sweep_rounds")
    assert all(t == "window" for d in mc.paths(c)["dirs"] for t, _, _ in d)
    for bw in (False, True):                                   # dense: every wave's farthest neighbour is inside the first radius
        assert max(float(w["d"].max()) for w in wave_view(c, recs[0], 0, bw)) < 0.15 * 0.9995
    for bw in (False, True):                                   # lattice: every neighbour is 0.25 m off, beyond the first radius,
        ws = wave_view(c, recs[1], 1, bw)                      # and every wave has seen a target in round one (a finite worst)
        assert all((w["d"] == F(0.25)).all() and gap(w) == 0.0 for w in ws)
    for bw in (False, True):                                   # far: no target within 0.15 * 4^3 m along u of any wave: the radius
        ws = wave_view(c, recs[2], 2, bw)                      # quadruples at least four times; the neighbours are ~36 m off
        assert min(gap(w) for w in ws) > 9.6 + 0.1 and min(float(w["d"].min()) for w in ws) > 30.0
    (w,) = wave_view(c, recs[3], 3, False)                     # outlier: one wave, 63 rows settled in round one, one 3.9 m off
    assert len(w["d"]) == 64 and int((w["d"] < 0.15).sum()) == 63 and float(w["d"].max()) > 3.0


def test_shapes_by_numbers():
    assert lens(mc.get("scan_q2_N1025"))[0] == (1025, 1025) and 1025 - mc.SCAN_TILE == 1          # ONE row in the last tile
    assert lens(mc.get("scan_q2_N2048"))[0] == (2048, 2 * mc.SCAN_TILE)
    q4 = lens(mc.get("scan_q4_B129_N1025"))
    assert q4[:3] == [(1025, 1025), (1025, 1), (17, 1024)] and all(1 <= n <= 20 for p in q4[3:] for n in p) and 129 * 1025 < 1 << 18
    assert lens(mc.get("scan_N16385")) == [(16385, 40)]
    assert [n2 for _, n2 in lens(mc.get("sweep_nt_1_15_16_17"))] == [1, 15, 16, 17]
    plain = lens(mc.get("sweep_plain_B256_N1024"))
    assert sum(min(p) >= 200 for p in plain) == 4 and all(max(p) <= 5 for p in plain[4:])
    sw = lens(mc.get("sweep_shared_window"))
    assert sorted({n1 - 512 for n1, _ in sw}) == [1, 64, 65] and sorted({n2 for _, n2 in sw}) == [511, 512, 2049]
    p = mc.paths(mc.get("sweep_shared_window"))["dirs"]
    assert [d[0][0] for d in p] == ["window", "shared", "shared"] * 2 + ["window"] * 3             # 511 targets, 65 rows: the negatives
    fs = mc.get("sweep_fullscan")
    p = mc.paths(fs)["dirs"]
    for (n1, n2), d in zip(lens(fs), p):
        want = lambda nq, nt: ("full", 8 if nq == 40 else 4) if (nq in (40, 300) and nt >= 512) else ("window", 1)     # noqa: E731
        assert d[0][:2] == want(n1, n2) and d[1][:2] == want(n2, n1), (n1, n2, d)
    # 513 targets are 33 chunks; over 8 shares of ceil(33 / 8) = 5 chunks the seventh is short and the eighth empty
    per = -(-33 // 8)
    assert [max(0, min(per, 33 - s * per)) for s in range(8)] == [5, 5, 5, 5, 5, 5, 3, 0]
    st = mc.paths(mc.get("sweep_staging_N4112"))["dirs"]
    assert [d[0][2] for d in st] == [True, False, True, True] and [d[1][2] for d in st] == [True, True, True, False]
    e = lens(mc.get("empty_and_one_point_N2049"))
    assert e == lens(mc.get("empty_and_one_point_N300")) == [(200, 0), (0, 200), (0, 0), (1, 1), (1, 200), (200, 1), (150, 170)]


def test_thin_box_keys():
    c = mc.get("sweep_thin_box_45")
    for a, b in zip(c["P1"], c["P2"]):
        assert mc.sort_code(a, b) < 3 and mc.sort_code(a, b, dir_keys=True) == 4          # "sort code >= 3" only where hist_icp sorted


def dev32(M):
    """the backward window's test of the pose, in the kernel's float32 operations"""
    M = np.asarray(M, F)
    dev = F(0)
    for a0 in range(3):
        for a1 in range(3):
            g = M[0, a0] * M[0, a1] + M[1, a0] * M[1, a1] + M[2, a0] * M[2, a1]
            dev = max(dev, abs(g - F(1.0 if a0 == a1 else 0.0)))
    return dev


def test_poses_by_numbers():
    devs = {n: dev32(M) for n, M in mc.pose_list()}
    assert all(devs[n] <= F(1e-4) for n in ("identity", "yaw_0.3", "yaw_179.9", "reflection", "scale_1.00004", "to_3km")), devs
    assert devs["scale_1.00006"] > F(1e-4) and devs["scale_1.05"] > F(1e-4) and devs["scale_1.00004"] > F(5e-5), devs
    M = dict(mc.pose_list())
    assert np.linalg.det(M["reflection"][:3, :3].astype(np.float64)) < -0.999
    assert abs(np.degrees(np.arctan2(M["yaw_179.9"][1, 0], M["yaw_179.9"][0, 0])) - 179.9) < 1e-3
    for name in ("poses_N300", "poses_N2049"):
        c = mc.get(name)
        recs, out = mc.restated(name)
        far = [n for n, _ in mc.pose_list()].index("to_3km")
        n1 = recs[far]["n1"]
        assert np.linalg.norm(np.array(recs[far]["So"]) / n1) < 10.0 and np.linalg.norm(np.array(recs[far]["Sm"]) / n1) > 3000.0
        assert (out["errors"] < 0.5).all() and (out["inliers"] > 0).all(), out["errors"]       # every pair registers under its pose


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("threshold")])
def test_threshold_rows_by_numbers(name):
    c = mc.get(name)
    recs, _ = mc.restated(name)
    th = F(c["thres"])
    sweep = mc.CASES[name]["kernel"].startswith("sweep")
    for b, (r1, r2, want) in enumerate(c["marks"]):
        assert want == [th, np.nextafter(th, F(0)), th, np.nextafter(th, F(0))]
        code, o1, o2 = mc.sorted_rows(c["P1"][b], c["P2"][b])
        for d, rows, o in ((0, r1, o1), (1, r2, o2)):
            assert [recs[b]["d"][d][i] for i in rows] == want, (name, b, d)                 # exactly at, one step inside
            assert [bool(recs[b]["inl"][d][i]) for i in rows] == [False, True, False, True]
            place = [int(np.flatnonzero(o == i)[0]) for i in rows] if sweep else rows        # the sorted rank, or the row
            assert [p % 256 // 64 for p in place] == [0, 0, 3, 3], (name, b, d, place)      # first and last wave of a block
            assert place[0] // 256 == 0 and place[3] == len(o) - 1 if sweep else True
    if "fullscan" in name:
        p = mc.paths(c)["dirs"]
        assert p[0][0][:2] == ("full", 8) and p[1][1][:2] == ("full", 8)                      # each direction is the shared one once


@pytest.mark.parametrize("name", ["duplicates_scan_N1100", "duplicates_sweep_N2049"])
def test_duplicates_by_numbers(name):
    c = mc.get(name)
    recs, _ = mc.restated(name)
    p2 = c["P2"][0]
    code, o1, o2 = mc.sorted_rows(c["P1"][0], p2)
    for k, (i, j) in enumerate(c["dup"]):
        assert np.array_equal(p2[i], p2[j])
        place = sorted(int(np.flatnonzero(o2 == x)[0]) for x in (i, j)) if "sweep" in name else [i, j]
        assert place == [[15, 16], [1023, 1024]][k]                                          # a chunk seam, the tile seam
        d = recs[0]["d"][0][k]                                                              # the moved row k of pcd1 lies 1 mm off in x, y, z
        assert abs(float(d) - 0.001 * np.sqrt(3)) < 2e-5 and d == np.sqrt(mr.sqdist(recs[0]["mv"][k], p2[i, :3]))


def test_rotation_cases_by_numbers():
    names, Ts = mc.rotation_poses()
    r = {n: mr.rotations32(M) for n, M in zip(names, Ts)}
    assert np.isnan(r["m8_above_1"][1]) and np.isnan(r["m8_below_minus_1"][1])
    assert not np.isnan(r["m8_above_1"][[0, 2]]).any() and not np.isnan(r["m8_below_minus_1"][[0, 2]]).any()
    assert r["half_turn_plus_zero"][0] == F(180.0) and r["half_turn_minus_zero"][0] == F(-180.0)
    assert np.array_equal(mc.get("rotations_exact_N16")["names"], names)


def test_fullscan_last_targets_by_numbers():
    """row 0 of either cloud has the LAST row of the other side's sorted order as its nearest neighbour, 1 mm off"""
    c = mc.get("sweep_fullscan")
    recs, _ = mc.restated("sweep_fullscan")
    for b, r in enumerate(recs):
        code, o1, o2 = mc.sorted_rows(c["P1"][b], c["P2"][b])
        assert code == 0
        last2, last1 = c["P2"][b][o2[-1], :3], r["mv"][o1[-1]]
        assert r["d"][0][0] == np.sqrt(mr.sqdist(r["mv"][0], last2)) and r["d"][0][0] < 0.002, (b, r["d"][0][0])
        assert r["d"][1][0] == np.sqrt(mr.sqdist(c["P2"][b][0, :3], last1)) and r["d"][1][0] < 0.002, (b, r["d"][1][0])


def test_shrinking_pose_by_numbers():
    c = mc.get("sweep_scale_0.95_window")
    (r,), _ = mc.restated("sweep_scale_0.95_window")
    p1, p2, M = c["P1"][0], c["P2"][0], c["T"][0]
    assert dev32(M) > F(1e-4)                                                        # the window must be the whole cloud
    code, o1, o2 = mc.sorted_rows(p1, p2)
    assert code == 0 and o2[-1] == r["n2"] - 1 and o1[-1] == r["n1"] - 1 and (r["n1"] - 1) % 16 == 0
    q = r["n2"] - 1                                                                  # the query: last in its cloud's order
    d = np.sqrt(mr.sqdist(p2[q, :3], r["mv"]))
    assert abs(d[-1] - 0.12) < 1e-5 and abs(d[-2] - 0.14) < 1e-5 and r["d"][1][q] == d[-1] and np.sort(d)[2] > 0.5
    assert d[-2] < 0.15 * 0.9995
    w = wave_view(c, r, 0, True)[-1]                                                 # its wave: nobody's neighbour beyond the first radius,
    assert np.sort(w["d"])[-2] < 0.14 and w["cu"].max() == w["cu"][-1]             # and the query is the wave's upper end
    slack = 2e-3 + 2e-5 * (abs(float(w["cu"].min())) + abs(float(w["cu"].max())))
    assert float(w["tk"][-1] - w["cu"][-1]) > 0.15 + slack + 0.01 and float(w["tk"][-2] - w["cu"][-1]) < 0.15
    assert float(w["cu"].min()) - 0.15 < float(w["tk"][0]) + 1.0 and float(w["tk"][-3]) < float(w["cu"][-1])     # (the cloud's own rows are inside)


@pytest.mark.parametrize("N", [300, 2049])
def test_hist_icp_eval_batch_by_numbers(N):
    S, D = mc.hist_icp_eval_batch(N)
    assert S.shape == D.shape == (12, N, 4)
    pairs = [sr.axis_sorted_pair(s, d, dir_keys=True) for s, d in zip(S, D)]
    swaps = [p["swap"] for p in pairs]
    assert 3 <= sum(swaps) <= 9                                                      # both swap states
    codes = [p["code"] for p in pairs]
    assert (codes[10:] == [4, 4] and swaps[10:] == [0, 1]) if N == 2049 else all(c < 3 for c in codes)     # direction keys, either role fixed
    if N == 2049:       # the reuse path's sweeps take every branch: shared full scans, shared windows, plain windows
        t = {mc.direction_path(a, b, 12, N)[0] for p in pairs for a, b in ((p["nA"], p["nC"]), (p["nC"], p["nA"]))}
        assert t == {"full", "shared", "window"}

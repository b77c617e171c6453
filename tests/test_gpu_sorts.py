"""The sorts on their own: what zsort_kernel, sort_clouds_body (1024 threads in sort_clouds_kernel, 512 in front_roles_kernel),
sort_code_kernel, chunk_sort_kernel and chunk_merge_kernel leave in the caller's workspace, against tests/sort_restatement.py --
exactly: a stable order by (key, row) of keys that NumPy restates bit for bit.  Only the points a pre-pose has moved get a bound.

Every call runs on an exactly sized workspace filled with NaNs (tests/sort_device.py), and every array is first shown to have
been written (no poison in the rows judged), so a path that skipped its sort fails.  Inputs: tests/sort_cases.py; that they hold
the ties, margins and thresholds their names claim is asserted on the CPU (tests/test_sort_restatement.py).

Which call reaches which sort (csrc/api.hip hist_icp_core, run_init_pose, csrc/icp.hip launch_icp):
  hist_icp, N <= 4096     zsort_kernel counting for itself; the axis sort in the vote's launch (512 threads), or with no_front_roles
                          sort_clouds_kernel counting for itself on the side stream, or with no_side_stream on the caller's stream
                          with the lengths of the z-sort -- for N > 2048 in front of the scoring, raw; for N <= 2048 the first sort
                          of that path is launch_icp's, which carries the initial pose (a translation) as its pre-pose: there the
                          moving role is judged like any pre-posed cloud and only the fixed role can equal the other paths' bits
  hist_icp, N > 4096      count_pair's boxes; chunked z-sort; chunked axis sort behind sort_code_kernel, with no_dir_keys the boxed branch
  apply_icp / icp         the axis sort with a pre-pose (NULL for icp), boxes NULL: sort_clouds_kernel up to 4096, beyond it
                          sort_code_kernel, or fixed_axis in every chunk with no_dir_keys
  init_pose               the z-sort without boxes (vote_key_params in every chunk)
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import sort_cases as sc          # noqa: E402
import sort_device as sd         # noqa: E402
import sort_restatement as sr    # noqa: E402

F = np.float32
U = 2.0 ** -24
_worst_pose = [0.0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def ids_of(rows):
    return np.ascontiguousarray(rows[:, 3]).view(np.int32)


def check_order(code, rows, what):
    """keys recomputed from the OUTPUT coordinates: non-decreasing, ids ascending inside every run of equal canonical keys"""
    k = sr.canonical(sr.axis_key(code, rows[:, :3]))
    ids = ids_of(rows)
    dk = np.diff(k)
    assert (dk >= 0).all(), f"{what}: keys decrease at rows {np.flatnonzero(dk < 0)[:5]}"
    tie = dk == 0
    assert (np.diff(ids)[tie] > 0).all(), f"{what}: ids do not ascend inside a run of equal keys at rows {np.flatnonzero(tie & (np.diff(ids) <= 0))[:5]}"


def check_axis(res, S, D, dir_keys=True, swap_allowed=True, pose=None, xsoa=True, moving_posed=False, names=None):
    """Every assertion about an axis-sorted batch.  pose [B, 4, 4]: the pre-pose of the moving role; moving_posed: a pre-pose this
    test does not know (a translation) -- the moving role then shows a permutation in key order, moved by one constant.
    The bound of a posed point: xf_apply forms, per component, one product, two fmaf and the sum with t -- four roundings, each
    relative to a partial sum bounded by (|R| |p| + |t|)_r, and (1 + u)^4 - 1 < 5 u:  |got - pose . p| <= 5 . 2^-24 (|R| |p| + |t|)_r,
    the bound of test_transform_points_within_the_rounding_bound for the same four operations."""
    B, N, NP16 = res.B, res.N, res.NP16
    out = []
    for b in range(B):
        tag = f"pair {b}" + (f" ({names[b]})" if names else "")
        w = sr.axis_sorted_pair(S[b], D[b], dir_keys=dir_keys, swap_allowed=swap_allowed)
        assert (res.lenA[b], res.lenC[b]) == (w["nA"], w["nC"]), tag
        if res.entry == "hist_icp":
            assert res.swap[b] == w["swap"], tag
        assert res.axis[b] == w["code"], (tag, int(res.axis[b]), w["code"], w["info"])
        fixed, moving = (S[b], D[b]) if w["swap"] else (D[b], S[b])
        for role, arr, soa, cloud, n, want_ids in (("fixed", res.pts, res.sortYsoa, fixed, w["ny"], w["fixed_ids"]),
                                                   ("moving", res.sortX, res.sortXsoa if xsoa else None, moving, w["nx"], w["moving_ids"])):
            what = f"{tag} {role} role ({n} rows, code {w['code']})"
            rows = arr[b, :n]
            assert not sd.poisoned(rows), f"{what}: poison left in the first n rows: the sort did not write them"
            ids = ids_of(rows)
            assert np.array_equal(np.sort(ids), np.arange(n)), f"{what}: ids are no permutation of 0 .. n - 1"
            if role == "moving" and pose is not None:
                Rm, t = pose[b, :3, :3].astype(np.float64), pose[b, :3, 3].astype(np.float64)
                p = cloud[ids, :3].astype(np.float64)
                bound = 5 * U * (np.abs(p) @ np.abs(Rm).T + np.abs(t))
                ratio = np.abs(rows[:, :3].astype(np.float64) - (p @ Rm.T + t)) / bound
                if n:
                    _worst_pose[0] = max(_worst_pose[0], float(ratio.max()))
                    assert (ratio <= 1.0).all(), (what, float(ratio.max()))
            elif role == "moving" and moving_posed:
                # a translation t as the pre-pose: the products with the identity's entries are exact, so got = fl(p + t), one
                # rounding: got - p = t + e, |e| <= 2^-24 |got|, and over the rows of a pair got - p spreads by at most 2 . 2^-24 max |got|
                if n:
                    d = rows[:, :3].astype(np.float64) - cloud[ids, :3].astype(np.float64)
                    assert ((d.max(axis=0) - d.min(axis=0)) <= 2 * U * np.abs(rows[:, :3].astype(np.float64)).max(axis=0)).all(), what
            else:
                assert np.array_equal(bits(rows[:, :3]), bits(cloud[ids, :3])), f"{what}: a row is not its input row bit for bit"
                assert np.array_equal(ids, want_ids), f"{what}: order differs from the restatement at rows {np.flatnonzero(ids != want_ids)[:5]}"
            check_order(w["code"], rows, what)
            if soa is not None:
                assert not sd.poisoned(soa[b]), f"{what}: poison left in the structure-of-arrays image"
                assert np.array_equal(bits(soa[b, :, :n].T), bits(rows[:, :3])), f"{what}: structure-of-arrays image differs from the rows"
                assert np.array_equal(bits(soa[b, :, n:NP16]), bits(np.full((3, NP16 - n), np.inf, F))), f"{what}: padding of the image is not +inf"
        out.append(w)
    return out


def check_z(res, S, D, names=None):
    B, N = res.B, res.N
    recs = []
    for b in range(B):
        tag = f"pair {b}" + (f" ({names[b]})" if names else "")
        rec = sr.vote_key_record(S[b], D[b], res.h_box)
        assert not sd.poisoned(res.voteKey[b, :5]), tag
        assert np.array_equal(res.voteKey[b, :5], np.array(rec, F)), (tag, res.voteKey[b, :5], rec)
        assert (res.lenA[b], res.lenC[b]) == (sr.length(S[b]), sr.length(D[b])), tag
        for cloud, arr, which in ((S[b], res.zsortA[b], "src"), (D[b], res.zsortC[b], "dst")):
            n, rows = sr.z_sorted_cloud(cloud, rec)
            what = f"{tag} {which} cloud by the vote's key ({n} rows, wide {rec[0]})"
            assert not sd.poisoned(arr[:n]), f"{what}: poison left in the first n rows"
            bad = np.flatnonzero((bits(arr[:n]) != bits(rows)).any(axis=1))
            assert len(bad) == 0, f"{what}: rows {bad[:5]} differ from the flagged input rows in restated order (key in w)"
            if N <= 4096:
                assert np.array_equal(bits(arr[n:]), bits(np.tile(np.array([0, 0, np.inf, np.inf], F), (N - n, 1)))), f"{what}: rows behind n"
            else:      # sort.hip: the chunked merge leaves the rows behind n unwritten
                assert (bits(arr[n:]) == sd.POISON_WORD).all(), f"{what}: the chunked merge wrote rows behind n"
        recs.append(rec)
    return recs


def same_first_rows(a, b, S, D, moving=True, what=""):
    """two runs left identical arrays on the first n rows of every role and cloud"""
    for k in range(a.B):
        nA, nC, swap, _, nx, _, ny = sr.roles(S[k], D[k])
        assert a.axis[k] == b.axis[k] and a.swap[k] == b.swap[k] and a.lenA[k] == b.lenA[k] and a.lenC[k] == b.lenC[k], (what, k)
        assert np.array_equal(bits(a.pts[k, :ny]), bits(b.pts[k, :ny])), (what, k, "fixed role")
        assert np.array_equal(bits(a.sortYsoa[k][:, :ny]), bits(b.sortYsoa[k][:, :ny])), (what, k)
        if moving:
            assert np.array_equal(bits(a.sortX[k, :nx]), bits(b.sortX[k, :nx])), (what, k, "moving role")
            assert np.array_equal(bits(a.sortXsoa[k][:, :nx]), bits(b.sortXsoa[k][:, :nx])), (what, k)
        assert np.array_equal(bits(a.zsortA[k, :nA]), bits(b.zsortA[k, :nA])) and np.array_equal(bits(a.zsortC[k, :nC]), bits(b.zsortC[k, :nC])), (what, k)
        assert np.array_equal(bits(a.voteKey[k, :5]), bits(b.voteKey[k, :5])), (what, k)


def poses(B, seed=0):
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (B, 1, 1))
    for b in range(B):
        a = np.deg2rad(rng.uniform(-20, 20))
        T[b, :3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        T[b, :3, 3] = rng.uniform(-1.5, 1.5, 3)
    return T.astype(F)


@pytest.mark.parametrize("N", [1024, 1025, 4096])
def test_seams_of_the_single_workgroup_network(N):
    """Counts 0, 1, 2, 63, 64, 65, 127, 129, 511, 513, 1023, 1024 and N in one ragged batch, through the three front paths of
    icpflow_hist_icp (max_iterations = 1) on the same inputs; all three leave the same bits on the first n rows."""
    S, D = sc.seam_batch(N)
    raw_on_stream = N > 2048      # (no_side_stream: see the module's table)
    front = sd.run("hist_icp", S, D)
    check_axis(front, S, D)
    check_z(front, S, D)
    side = sd.run("hist_icp", S, D, no_front_roles=True)
    check_axis(side, S, D)
    check_z(side, S, D)
    own = sd.run("hist_icp", S, D, no_side_stream=True)
    check_axis(own, S, D, xsoa=raw_on_stream, moving_posed=not raw_on_stream)
    check_z(own, S, D)
    same_first_rows(front, side, S, D, what="front roles / side stream")
    same_first_rows(front, own, S, D, moving=raw_on_stream, what="front roles / caller's stream")


@pytest.mark.parametrize("N", [4097, 8200])
def test_seams_of_the_chunked_sort(N):
    """Counts 0, 1, 65, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145 (those that fit) and N: the vote's z-sort and the axis
    sort with and without direction keys (boxes given), and the un-boxed sorts of icpflow_icp and of icpflow_apply_icp's pre-pose."""
    S, D = sc.seam_batch(N)
    for no_dir in (False, True):
        r = sd.run("hist_icp", S, D, no_dir_keys=no_dir)
        w = check_axis(r, S, D, dir_keys=not no_dir)
        check_z(r, S, D)
        assert not no_dir or all(x["code"] <= 2 for x in w)
        r = sd.run("apply_icp", S, D, init=poses(len(S), N), no_dir_keys=no_dir)
        check_axis(r, S, D, dir_keys=not no_dir, swap_allowed=False, pose=poses(len(S), N), xsoa=False)
    check_axis(sd.run("icp", S, D), S, D, swap_allowed=False, xsoa=False)
    check_z(sd.run("init_pose", S, D), S, D)
    print(f"N = {N}: pre-posed points, max |got - pose . p| / bound = {_worst_pose[0]:.3f}")


@pytest.mark.parametrize("N", [1025, 4096])
def test_pre_pose_in_one_workgroup(N):
    """icpflow_apply_icp below and at 4096: sort_clouds_kernel with the initial poses as the pre-pose of the moving (src) cloud."""
    S, D = sc.seam_batch(N, seed=1)
    T = poses(len(S), N)
    check_axis(sd.run("apply_icp", S, D, init=T), S, D, swap_allowed=False, pose=T, xsoa=False)
    check_axis(sd.run("icp", S, D), S, D, swap_allowed=False, xsoa=False)
    print(f"N = {N}: pre-posed points, max |got - pose . p| / bound = {_worst_pose[0]:.3f}")


def test_chunked_equals_single():
    """The valid rows of an N = 4096 batch in an N = 4097 batch, one more pad row: sort.hip's "identical to the single-workgroup
    kernels'" -- first n rows, ids, codes and vote keys of the two runs are the same bits.  Seam counts, the key-choice clouds
    (direction codes) and the walls (the wide vote key)."""
    for make, ez in ((lambda N: sc.seam_batch(N), None), (lambda N: sc.key_choice_batch(N)[:2], None), (lambda N: sc.wide_batch(N)[:2], sc.WIDE_EZ)):
        S, D = make(4096)
        S2, D2 = sc.rebatch(S, D, 4097)
        one, many = sd.run("hist_icp", S, D, ez=ez), sd.run("hist_icp", S2, D2, ez=ez)
        check_axis(one, S, D)
        check_axis(many, S2, D2)
        check_z(one, S, D)
        check_z(many, S2, D2)
        same_first_rows(one, many, S, D, what="single / chunked")


@pytest.mark.parametrize("N", [4096, 8200])
def test_ties(N):
    """Three keys over 6000 rows (runs of equal keys across the chunk seams), one key, duplicated points, +0.0 and -0.0 interleaved,
    denormal keys, keys near +-3000 m and +-1e6 m -- under the axis key and under z, boxed (hist_icp) and un-boxed (icp, init_pose)."""
    S, D, names, _ = sc.ties_batch(N)
    r = sd.run("hist_icp", S, D)
    check_axis(r, S, D, names=names)
    check_z(r, S, D, names=names)
    check_axis(sd.run("icp", S, D), S, D, swap_allowed=False, xsoa=False, names=names)
    r = sd.run("init_pose", S, D)
    check_z(r, S, D, names=names)
    check_axis(r, S, D, dir_keys=False, swap_allowed=False, names=names)     # (N > 2048: the entry sorts for its scoring sweeps)


@pytest.mark.parametrize("N", [2048, 4097])
def test_key_choice(N):
    """The thin box turned 45 degrees (code 4), the same box axis-aligned, a cube (extents equal on three axes) and a box with
    e1 = e2 > e0 as fixed clouds at ny = 1024 / 1025 and nx = 511 / 512: through the 512-thread front role, through
    sort_clouds_kernel (no_front_roles; icpflow_icp) and chunked through sort_code_kernel; no_dir_keys leaves codes <= 2."""
    S, D, names, want = sc.key_choice_batch(N)
    runs = [sd.run("hist_icp", S, D)] + ([sd.run("hist_icp", S, D, no_front_roles=True)] if N <= 4096 else [])
    for r in runs:
        w = check_axis(r, S, D, names=names)
        for b, (name, kind) in enumerate(zip(names, want)):
            assert (r.axis[b] == 4) == (kind == "direction"), (name, int(r.axis[b]))
            assert kind == "direction" or r.axis[b] == w[b]["info"]["legacy"], name
        check_z(r, S, D, names=names)
    w = check_axis(sd.run("icp", S, D), S, D, swap_allowed=False, xsoa=False, names=names)
    assert w[0]["code"] == 4 and w[3]["code"] == 4 and w[1]["code"] <= 2 and w[2]["code"] <= 2
    r = sd.run("hist_icp", S, D, no_dir_keys=True)
    check_axis(r, S, D, dir_keys=False, names=names)
    assert (r.axis <= 2).all()


@pytest.mark.parametrize("N", [4096, 4097])
def test_wide_vote_key(N):
    """A wall 40 m along x and 3 m high with 4097 rows in both clouds together (wide) and with 4096 (plain z), along y (uaxis 1),
    8 m less and more one float32 step, a z range of exactly 250 h (plain z) and just below; rows on slab borders
    ((z - z0) / h an integer exactly, h = 0.25).  One workgroup per cloud at 4096, chunked with boxes (hist_icp) and without
    (init_pose) at 4097."""
    S, D, names, want = sc.wide_batch(N)
    for entry in ("hist_icp", "init_pose"):
        r = sd.run(entry, S, D, ez=sc.WIDE_EZ)
        recs = check_z(r, S, D, names=names)
        assert [rec[:2] for rec in recs] == want
        assert [(int(k[0]), int(k[1])) for k in r.voteKey] == want


@pytest.mark.parametrize("N", [1025, 4097])
def test_reruns_and_a_second_stream_leave_the_same_bits(N):
    """Two runs on the caller's stream and one on a second stream: every array of the layout the same bytes.  (Floats 5 .. 7 of a
    vote-key record are written from words of LDS that nobody sets and nobody reads: left out.)"""
    S, D = sc.seam_batch(N, seed=2)
    a = sd.run("hist_icp", S, D)
    b = sd.run("hist_icp", S, D)
    side = torch.cuda.Stream()
    c = sd.run("hist_icp", S, D, stream=side)
    check_axis(a, S, D)
    check_z(a, S, D)
    for other in (b, c):
        for name in sd.LAYOUT:      # (whole arrays, the poison a sort leaves behind the valid rows included; of a vote key its five numbers)
            x, y = (getattr(r, name)[:, :5] if name == "voteKey" else getattr(r, name) for r in (a, other))
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name

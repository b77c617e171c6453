"""CPU-only: every input of tests/ego_map_cases.py is the case its name claims -- in numbers: the home slots and the loads of
the tables, the seam positions, the exact equalities at the crop's, the prune's and the gate's edges, the float32-versus-fp64
voxel flips, and, for the registration's decisions, that each single wrong decision moves the pose by more than 1e-3 m or
1e-4 rad.  Also: the restatement (tests/ego_motion_restatement.py) gives the answer that can be checked by hand on the smallest
cases.  Figures are printed (run with -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_map_cases as cases            # noqa: E402
import ego_motion_restatement as rest    # noqa: E402

F = np.float32
MARGIN_M, MARGIN_RAD = 1e-3, 1e-4
_made = {}


def made(table, name):
    if name not in _made:
        _made[name] = table[name]()
    return _made[name]


def test_home_is_the_kernels_hash_in_uint64():
    """by hand: key 1 -> the upper half of the constant; the product wraps at 2^64"""
    assert int(cases.home(np.array([1]), 1023)[0]) == (0x9E3779B97F4A7C15 >> 32) & 1023
    k = (1 << 62) + 12345
    assert int(cases.home(np.array([k], np.uint64), 0xFFFF)[0]) == (((k * 0x9E3779B97F4A7C15) % (1 << 64)) >> 32) & 0xFFFF
    _, h = cases.grid()
    per_slot = np.bincount(h, minlength=1024)
    print(f"voxels of [-57, 57]^3 per home slot of a 1024 table: {per_slot.min()} .. {per_slot.max()}")
    assert per_slot.min() >= 575 and per_slot.max() <= 1955


# ============================================================================================ A
@pytest.mark.parametrize("name,slot", [("chain_40", 500), ("chain_40_wrap", 1023)])
def test_chain_shares_one_home(name, slot):
    c = made(cases.MAP_CASES, name)
    (first, _), (second, _) = c["frames"]
    k0, k1 = cases.keys_of(first, 1.0), cases.keys_of(second, 1.0)
    assert len(np.unique(k0)) == 40 and sorted(k0) == sorted(k1) and not np.array_equal(k0, k1)
    assert (cases.home(k0, cases.MASK) == slot).all() and (slot == cases.MASK) == (name == "chain_40_wrap")   # 40 from slot 1023: wraps
    assert (np.linalg.norm(first.astype(np.float64), axis=1) < 100.0).all()
    snaps = cases.restated_maps(c)
    assert all(len(v) == 1 for v in snaps[0].values())
    for k, p in zip(k0.tolist(), first):
        assert np.array_equal(snaps[1][k], np.stack([p, second[k1 == k][0]]))        # first frame's point, then the second's


def test_chain_pruned_middle_drops_every_second_voxel():
    c = made(cases.MAP_CASES, "chain_pruned_middle")
    k = cases.keys_of(c["frames"][0][0], 1.0)
    assert (cases.home(k, cases.MASK) == 300).all() and len(np.unique(k)) == 30
    d = np.linalg.norm(c["frames"][0][0].astype(np.float64) - (60.0, 0.0, 0.0), axis=1)
    assert (d[0::2] < 100.0).all() and (d[1::2] > 100.0).all()
    snaps = cases.restated_maps(c)
    assert len(snaps[0]) == 30
    assert sorted(snaps[1]) == sorted(k[0::2].tolist() + cases.keys_of(c["source"][15:], 1.0).tolist()) and len(snaps[1]) == 20
    pose, iterations, last, ncorr = rest.register(c["source"], c["_map"].arrays(), c["guess"], c["sigma"], 1.0, 1)
    assert (iterations, last, ncorr) == (1, 0.0, 20) and np.array_equal(pose, np.eye(4))


@pytest.mark.parametrize("name,count", [("load_half", 512), ("load_full", 1024)])
def test_load(name, count):
    c = made(cases.MAP_CASES, name)
    k = cases.keys_of(c["frames"][0][0], 1.0)
    assert len(np.unique(k)) == count and sorted(k) == sorted(cases.keys_of(c["frames"][1][0], 1.0))
    assert (np.linalg.norm(c["frames"][0][0].astype(np.float64), axis=1) < 100.0).all()
    worst = cases.longest_displacement(k, cases.MASK)
    print(f"{name}: {count} live voxels of 1024 slots, longest displacement of a sequential insertion {worst}")
    assert worst >= (5 if count == 512 else 100)
    assert len(cases.restated_maps(c)[1]) == count


def test_full_plus_one_is_one_voxel_too_many():
    c = cases.full_plus_one()
    p = c["points"]
    assert len(np.unique(cases.keys_of(p, 1.0))) == 1025 == len(p)
    assert rest.crop_mask(p, 1.0, 100.0).all()
    ds, src = rest.downsample(p, 1.0, 100.0, 1.0)
    assert np.array_equal(ds, np.arange(1025))


def test_coord_range():
    c = cases.coord_range()
    lim = (1 << 20) - 2
    assert rest.crop_mask(c["beyond"], 1.0, 100.0).all() and np.floor(c["beyond"][0, 0].astype(np.float64) / 0.5e-4) >= lim
    for size in (0.5e-4, 1e-4, 1.5e-4):
        assert np.abs(np.floor(c["good"].astype(np.float64) / size)).max() < lim
    assert rest.crop_mask(c["good"], 1.0, 100.0).all() and len(c["good"]) >= 250
    with np.errstate(invalid="ignore"):
        assert not rest.crop_mask(c["bad"], 1.0, 100.0).any()


# ============================================================================================ B
@pytest.mark.parametrize("per_voxel", [1, 3, 20])
def test_cap_one_frame(per_voxel):
    c = made(cases.MAP_CASES, f"cap_one_frame[{per_voxel}]")
    pts = c["frames"][0][0]
    inside = (rest.voxel_coords(pts, 1.0) == c["voxel"]).all(1)
    assert np.array_equal(np.nonzero(inside)[0], c["rows"]) and len(c["rows"]) == 25
    for k in range(1, 9):                                   # both sides of every 256-row tile
        assert 256 * k - 1 in c["rows"] and 256 * k in c["rows"]
    assert len(np.unique(pts[c["rows"]], axis=0)) == 25
    snap = cases.restated_maps(c)[0]
    assert np.array_equal(snap[int(rest.pack(c["voxel"]))], pts[c["rows"][:per_voxel]])
    assert max(len(v) for v in snap.values()) == per_voxel and len(snap) == 301


def test_cap_two_frames():
    c = made(cases.MAP_CASES, "cap_two_frames")
    (f0, _), (f1, _) = c["frames"]
    snaps = cases.restated_maps(c)
    rows = lambda f, v: f[(rest.voxel_coords(f, 1.0) == v).all(1)]      # noqa: E731
    kA, kB, kC = (int(rest.pack(c[n])) for n in "ABC")
    assert (len(rows(f0, c["A"])), len(rows(f1, c["A"]))) == (18, 5)
    assert (len(rows(f0, c["B"])), len(rows(f1, c["B"]))) == (22, 3)
    assert (len(rows(f0, c["C"])), len(rows(f1, c["C"]))) == (0, 20)
    assert np.array_equal(snaps[1][kA], np.concatenate([rows(f0, c["A"]), rows(f1, c["A"])[:2]]))
    assert np.array_equal(snaps[1][kB], rows(f0, c["B"])[:20]) and np.array_equal(snaps[0][kB], snaps[1][kB])
    assert np.array_equal(snaps[1][kC], rows(f1, c["C"])) and kC not in snaps[0]


def test_faces():
    c = made(cases.MAP_CASES, "faces[1.0]")
    pts = c["frames"][0][0]
    ijk = rest.voxel_coords(pts, 1.0)
    at = 0
    for axis in range(3):
        for k in cases.FACE_K:
            assert pts[at, axis] == k and ijk[at, axis] == k                          # on the face: the voxel above it
            assert pts[at + 1, axis] < k and ijk[at + 1, axis] == k - 1               # one float32 step below
            assert pts[at + 2, axis] > k and ijk[at + 2, axis] == k
            at += 3
        assert np.signbit(pts[at, axis]) and pts[at, axis] == 0 and ijk[at, axis] == 0    # -0.0 is in voxel 0
        at += 1
    assert at == len(pts) == 48
    # 0.3 is no float32 and no fp64: float32(k * 0.3) lies on either side of the face
    pts = made(cases.MAP_CASES, "faces[0.3]")["frames"][0][0]
    ijk = rest.voxel_coords(pts, 0.3)
    side = [int(ijk[16 * axis + 3 * j, axis]) - k for axis in range(3) for j, k in enumerate(cases.FACE_K)]   # (16 rows per axis)
    print("faces[0.3]: voxel of float32(k * 0.3) minus k, per axis and k:", side)
    assert set(side) == {-1, 0}


def test_rounding_flips():
    c = made(cases.MAP_CASES, "rounding_flips")
    pts, pose = c["frames"][0]
    x64 = rest.move(pose, pts)
    flips = (np.floor(x64) != np.floor(x64.astype(F).astype(np.float64))).any(1)
    print(f"rounding_flips: {int(flips.sum())} of {len(pts)} rows change their voxel when the moved point is rounded to float32")
    assert flips.sum() >= 5 and flips.all()
    assert abs(pose[0, 1]) > 0.5 and np.allclose(pose[0:3, 0:3] @ pose[0:3, 0:3].T, np.eye(3))


def test_prune_edge():
    c = made(cases.MAP_CASES, "prune_edge")
    max2 = 100.0 * 100.0
    assert (cases.prune_d2(c["on"]) == max2).all() and len(c["on"]) == 5
    assert (cases.prune_d2(c["beyond"]) > max2).all() and len(c["beyond"]) == 5
    assert (cases.prune_d2(c["beyond"]) - max2 < 2e-3).all()                         # one float32 step: 8 micrometres at 100 m
    out, inn = c["first_out"]
    assert cases.prune_d2(out) > max2 > cases.prune_d2(inn) and np.array_equal(rest.voxel_coords(out, 1.0), rest.voxel_coords(inn, 1.0))
    inn, out = c["first_in"]
    assert cases.prune_d2(out) > max2 > cases.prune_d2(inn) and np.array_equal(rest.voxel_coords(out, 1.0), rest.voxel_coords(inn, 1.0))
    assert np.abs(c["frames"][1][1][0:3, 3]).min() > 0
    snaps = cases.restated_maps(c)
    assert len(snaps[0]) == 12                                                         # nothing leaves at frame 0
    want = cases.keys_of(c["on"], 1.0).tolist() + [int(cases.keys_of(inn[None], 1.0)[0])]
    assert sorted(snaps[1]) == sorted(want)
    assert np.array_equal(snaps[1][want[-1]], np.stack([inn, out, out]))              # kept whole


def test_sizes():
    c = made(cases.MAP_CASES, "sizes")
    assert [len(p) for p, _ in c["frames"]] == [0, 1, 255, 256, 257, 1025]
    assert len(cases.restated_maps(c)[-1]) <= 512


# ============================================================================================ C
@pytest.mark.parametrize("n,chunk", zip(cases.DS_SEAM_N, (1, 1, 2, 3, 5)))
def test_ds_seams(n, chunk):
    c = made(cases.DS_CASES, f"ds_seams[{n}]")
    assert len(c["points"]) == n and c["chunk"] == chunk
    keys = cases.keys_of(c["points"], 0.5)
    _, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    _, oinv = np.unique(c["owner"], return_inverse=True)
    assert np.array_equal(inv[np.argsort(inv, kind="stable")], np.sort(inv)) and counts.min() >= 1 and counts.max() <= 4
    assert len(np.unique(np.stack([inv, oinv], 1), axis=0)) == len(counts)          # same owner <=> same voxel
    assert rest.crop_mask(c["points"], 1.0, 100.0).all()
    across = cases.straddling_voxels(c["owner"], chunk)
    print(f"ds_seams[{n}]: chunk {chunk}, {len(counts)} voxels, {len(across)} with rows in different chunks, e.g. {across[:10]}")
    assert len(across) >= 10
    ds, src = rest.downsample(c["points"], 1.0, 100.0, 1.0)
    assert len(ds) == len(counts) and len(src) < len(ds)


def test_ds_crop_edge():
    c = made(cases.DS_CASES, "ds_crop_edge")
    p = c["points"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]
        mask = rest.crop_mask(c["points"], 1.0, 100.0)
    on = c["kind"] == "on"
    assert sorted(r2[on].tolist()) == [1.0] * 3 + [10000.0] * 6
    assert not mask[on].any() and mask[c["kind"] == "inside"].all() and (c["kind"] == "inside").sum() == 9
    assert not mask[c["kind"] == "outside"].any() and not mask[c["kind"] == "bad"].any() and (c["kind"] == "bad").sum() == 5
    ds, _ = rest.downsample(c["points"], 1.0, 100.0, 1.0)
    assert set(np.nonzero(c["kind"] == "inside")[0]) <= set(ds.tolist())             # each alone in its voxel


@pytest.mark.parametrize("size", [0.5, 1.5])
def test_ds_collisions(size):
    c = made(cases.DS_CASES, f"ds_collisions[{size}v]")
    assert c["constants"]["max_points"] == 512 == len(c["points"])                   # tcap = 1024, half full
    keys = cases.keys_of(c["points"], size)
    assert len(np.unique(keys)) == 512
    h = cases.home(keys, 1023)
    assert (h == c["home"]).sum() == 300
    ds, src = rest.downsample(c["points"], 1.0, 100.0, 1.0)
    assert np.array_equal(ds, np.arange(512))
    if size == 1.5:
        assert np.array_equal(src, np.arange(512))
    print(f"ds_collisions[{size}v]: 300 of 512 keys start at slot {c['home']}; longest displacement {cases.longest_displacement(keys, 1023)}")


def test_ds_one_voxel_and_all_distinct():
    one = made(cases.DS_CASES, "ds_all_one_voxel")["points"]
    assert len(np.unique(cases.keys_of(one, 0.5))) == 1 and len(one) == 3000
    ds, src = rest.downsample(one, 1.0, 100.0, 1.0)
    assert ds.tolist() == [0] and src.tolist() == [0]
    each = made(cases.DS_CASES, "ds_all_distinct")["points"]
    assert len(np.unique(cases.keys_of(each, 1.5))) == 3000
    ds, src = rest.downsample(each, 1.0, 100.0, 1.0)
    assert np.array_equal(ds, np.arange(3000)) and np.array_equal(src, np.arange(3000))


# ============================================================================================ D
def d2_of(a, b):
    e = np.asarray(a, F).astype(np.float64) - np.asarray(b, F).astype(np.float64)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def offset_rank(src, q):
    """position of q's voxel in the search order around src"""
    d = rest.voxel_coords(q, 1.0) - rest.voxel_coords(src, 1.0)
    return [int(np.nonzero((rest.OFFSETS == o).all(1))[0][0]) for o in d]


@pytest.mark.parametrize("name", ["tie_voxels", "tie_insertion"])
def test_ties_are_exact_and_the_first_wins(name):
    c = made(cases.REG_CASES, name)
    assert np.array_equal(d2_of(c["ties"], c["winners"]), d2_of(c["ties"], c["losers"]))
    rw, rl = offset_rank(c["ties"], c["winners"]), offset_rank(c["ties"], c["losers"])
    if name == "tie_voxels":
        assert all(a < b for a, b in zip(rw, rl)), (rw, rl)
        assert sorted(np.abs(rest.voxel_coords(c["winners"], 1.0) - rest.voxel_coords(c["losers"], 1.0)).sum(1)) == [1, 1, 1, 3]
    else:
        assert rw == rl == [13] * 4                                                    # one voxel: the source's own
    trace = []
    cases.restated_registration(c, trace=trace)
    assert np.array_equal(trace[0]["q"][-4:], c["winners"].astype(np.float64)) and trace[0]["keep"].all()
    trace = []
    cases.restated_registration(c, trace=trace, **cases.WRONG["last minimum"])
    assert np.array_equal(trace[0]["q"][-4:], c["losers"].astype(np.float64))
    assert np.array_equal(trace[0]["q"][:-4], c["source"][:-4].astype(np.float64))     # the untied ones: themselves


def test_gate_edge_is_exact():
    c = made(cases.REG_CASES, "gate_edge")
    assert (3.0 * c["sigma"]) ** 2 == 2.25
    assert (d2_of(*c["on"]) == 2.25).all() and len(c["on"][0]) == 6
    assert d2_of(*c["below"])[0] == np.nextafter(2.25, 0.0)
    assert max(offset_rank(*c["on"]) + offset_rank(*c["below"])) < 27 and 13 not in offset_rank(*c["on"])
    assert cases.restated_registration(c)[3] == 7
    assert cases.restated_registration(c, **cases.WRONG["gate <="])[3] == 13


def test_only_27():
    far, adj = made(cases.REG_CASES, "only_27[two away]"), made(cases.REG_CASES, "only_27[adjacent]")
    for c, dist, found in ((far, 2, 6), (adj, 1, 10)):
        mp = c["frames"][0][0][-4:]
        assert (np.abs(rest.voxel_coords(mp, 1.0) - rest.voxel_coords(c["lonely"], 1.0)).max(1) == dist).all()
        assert (d2_of(mp, c["lonely"]) < 9.0).all()
        assert cases.restated_registration(c)[3] == found == c["expect"]
    assert cases.restated_registration(far, **cases.WRONG["a 28th voxel"])[3] == 10


def test_twentieth_point_is_the_nearest():
    c = made(cases.REG_CASES, "twentieth_point")
    trace = []
    cases.restated_registration(c, trace=trace)
    snap = c["_map"].snapshot()
    for v, q in zip(c["voxels"], trace[0]["q"][-4:]):
        cell = snap[int(rest.pack(v))]
        assert len(cell) == 20 and np.array_equal(cell[19].astype(np.float64), q)


def test_few_and_own_points():
    pose, iterations, last, ncorr = cases.restated_registration(made(cases.REG_CASES, "few[2]"))
    assert (iterations, last, ncorr) == (1, 0.0, 2) and np.array_equal(pose, cases.FEW_GUESS)
    c = made(cases.REG_CASES, "few[3]")
    pose, iterations, last, ncorr = cases.restated_registration(c)
    assert (iterations, ncorr) == (1, 3) and last > 0.1 and not np.array_equal(pose, cases.FEW_GUESS)
    s = c["source"].astype(np.float64)
    assert np.linalg.norm(np.cross(s[1] - s[0], s[2] - s[0])) > 10.0                    # not collinear
    pose, iterations, last, ncorr = cases.restated_registration(made(cases.REG_CASES, "own_points"))
    assert (iterations, last, ncorr) == (1, 0.0, 40) and np.array_equal(pose, np.eye(4))


def test_m_seams_and_iteration_cap():
    for m in cases.M_SEAMS:
        c = made(cases.REG_CASES, f"m_seams[{m}]")
        assert len(c["source"]) == m and cases.restated_registration(c)[3] == m
    three, free = (cases.restated_registration(made(cases.REG_CASES, f"cap_iterations[{k}]")) for k in (3, 500))
    print(f"cap_iterations: {three[1]} iterations under the cap of 3 (|dx| {three[2]:.2e}), {free[1]} without (|dx| {free[2]:.2e})")
    assert three[1] == 3 and three[2] > 1e-4 and 3 < free[1] < 500 and free[2] < 1e-4


def test_empty_source_and_pruned_map_run_one_iteration():
    """a source of no points, or a map pruned to nothing: the loop runs once and stops (1 iteration, 0 correspondences, the
    guess); only a map that has received nothing is 0 iterations"""
    c = made(cases.REG_CASES, "own_points")
    cases.restated_registration(c)
    g = cases.FEW_GUESS
    pose, iterations, last, ncorr = rest.register(np.zeros((0, 3), F), c["_arrays"], g, 1.0, 1.0, fresh=False)
    assert (iterations, last, ncorr) == (1, 0.0, 0) and np.array_equal(pose, g)
    empty = rest.VoxelMap(1.0, 20, 100.0).arrays()
    assert rest.register(c["source"], empty, g, 1.0, 1.0, fresh=False)[1:] == (1, 0.0, 0)
    assert rest.register(c["source"], empty, g, 1.0, 1.0)[1:] == (0, 0.0, 0)
    odo = rest.Odometry()
    odo.register_frame(c["source"])
    odo.register_frame((c["source"] * F(0.001)))                                        # cropped to nothing
    assert [(r["iterations"], r["correspondences"], len(r["idx_ds"])) for r in odo.records] == [(0, 0, 40), (1, 0, 0)]
    assert np.array_equal(odo.poses[1], np.eye(4))


@pytest.mark.parametrize("name", sorted(cases.EXPOSES))
def test_every_wrong_decision_moves_the_pose(name):
    """the condition on the inputs of group D: the pose a single wrong decision gives is more than 1e-3 m or 1e-4 rad from
    the right one, so that no such decision hides under the GPU test's bound"""
    c = made(cases.REG_CASES, name)
    right = cases.restated_registration(c)
    for w in cases.EXPOSES[name]:
        wrong = cases.restated_registration(c, **cases.WRONG[w])
        dt, dth = rest.pose_error(wrong[0], right[0])
        print(f"{name}: '{w}' moves the pose by {dt:.3e} m {dth:.3e} rad ({wrong[3]} / {right[3]} correspondences)")
        assert dt > MARGIN_M or dth > MARGIN_RAD

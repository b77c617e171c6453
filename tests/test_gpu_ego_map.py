"""GPU: the ego-motion estimator's voxel map on its own (csrc/ego.hip through utils_ego_motion.egomotion's pieces) against the
restatement tests/ego_motion_restatement.py, on the hand-built inputs of tests/ego_map_cases.py -- what each of them is, is
proven on the CPU by tests/test_ego_map_cases.py.

Maps and down-sampled lists are compared WITHOUT tolerance and without sorting inside a voxel: the keys, the counts, every
point of every voxel in insertion order bit for bit, zeros behind a voxel's count.  Registrations: iterations and
correspondences are equal; the pose is within POSE_BOUND of the restatement's, 4 x the largest difference measured over this
file on one MI355X, 2026-10-21 (each case prints its own; run with -s):

    largest |dt| 6.795e-15 m (m_seams[512]), largest rotation 2.524e-16 rad (cap_iterations[3]); bound 2.718e-14 m, 1.010e-15 rad

i.e. the last bits of fp64 sums added in another order -- and at least 10^6 below the 1e-3 m / 1e-4 rad by which every single
wrong decision (the last minimum for the first, `<=` at the gate, a 28th voxel, a 20th point ignored) moves the pose of the
case that is there to expose it (asserted on the CPU).

Run on the MI355X box:  python -m pytest tests/test_gpu_ego_map.py -m gpu -q
"""
import os
import sys
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_map_cases as cases            # noqa: E402
import ego_motion_restatement as rest    # noqa: E402
from icp_flow_amd import utils_ego_motion  # noqa: E402

F = np.float32
POSE_BOUND_M, POSE_BOUND_RAD = 4 * 6.795e-15, 4 * 2.524e-16
_made, _first = {}, {}
_worst = [0.0, 0.0]


def made(table, name):
    """the case and the restatement's answer to it, built once"""
    if name not in _made:
        c = table[name]()
        if table is cases.MAP_CASES:
            c["_snaps"] = cases.restated_maps(c)
        elif table is cases.REG_CASES:
            c["_want"] = cases.restated_registration(c)
        _made[name] = c
    return _made[name]


def state(constants):
    return utils_ego_motion.egomotion(None, "cuda:0", **constants)


def export(ego):
    return tuple(t.cpu().numpy() for t in ego.map_export())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_map(got, want, what):
    """got: map_export's (keys, counts, points); want: {key: float32 [c,3]}"""
    keys, counts, pts = got
    assert keys.tolist() == sorted(want), (what, len(keys), len(want))
    for v, k in enumerate(keys.tolist()):
        c = int(counts[v])
        assert c == len(want[k]), (what, k, c, len(want[k]))
        assert np.array_equal(bits(pts[v, :c]), bits(want[k])), (what, k, pts[v, :c], want[k])      # insertion order, bit for bit
        assert not bits(pts[v, c:]).any(), (what, k)


def run_map(ego, c):
    """-> the export after every frame"""
    out = []
    for pts, pose in c["frames"]:
        ego.map_add(pts, pose)
        out.append(export(ego))
    return out


def run_registration(ego, c):
    for pts, pose in c["frames"]:
        ego.map_add(pts, pose)
    return ego.register_step(c["source"], c["guess"], c["sigma"]).cpu().numpy()


def run_downsample(ego, c):
    return tuple(t.cpu().numpy() for t in ego.downsample(c["points"]))


def check_registration(name, res, want, exact_pose=False):
    pose, iterations, last, ncorr = want
    dt, dth = rest.pose_error(res[0:16].reshape(4, 4), pose)
    print(f"{name}: GPU - restatement {dt:.3e} m {dth:.3e} rad; iterations {int(res[16])} / {iterations}; "
          f"final |dx| {res[17]:.3e} / {last:.3e}; correspondences {int(res[18])} / {ncorr}")
    _worst[0], _worst[1] = max(_worst[0], dt), max(_worst[1], dth)
    assert (int(res[16]), int(res[18])) == (iterations, ncorr), name
    assert res[12:16].tolist() == [0.0, 0.0, 0.0, 1.0] and res[19] == 0.0
    assert dt <= POSE_BOUND_M and dth <= POSE_BOUND_RAD, (name, dt, dth)
    if exact_pose:
        assert np.array_equal(res[0:16].reshape(4, 4), pose) and res[17] == last, name


# ============================================================================================ A, B: the map
@pytest.mark.parametrize("name", list(cases.MAP_CASES))
def test_map_equals_the_restatement(name):
    """map_add of every frame, map_export after each: the restatement's voxels, counts and points in insertion order.  Where
    the case has a source (chain_pruned_middle, load_*): every source point finds its map point again -- the count of
    correspondences -- and, all residuals being 0, the pose is the guess bit for bit"""
    c = made(cases.MAP_CASES, name)
    ego = state(c["constants"])
    got = run_map(ego, c)
    _first[name] = got
    for j, (g, w) in enumerate(zip(got, c["_snaps"])):
        assert_map(g, w, (name, j))
    print(f"{name}: frames of {[len(p) for p, _ in c['frames']]} points -> {[len(g[0]) for g in got]} voxels")
    if "source" in c:
        want = rest.register(c["source"], c["_map"].arrays(), c["guess"], c["sigma"], 1.0, 1, fresh=False)
        assert want[3] == len(c["source"])
        res = ego.register_step(c["source"], c["guess"], c["sigma"]).cpu().numpy()
        check_registration(name, res, want, exact_pose=True)
    ego.close()


def test_full_plus_one_is_a_status_and_reset_recovers():
    """1025 voxels for 1024 slots through register_frame: ICPFLOW_E_LIMIT, "a voxel table is full".  After reset() the state
    registers chain_40's first frame twice (the second registration has no residual: the identity, bit for bit, here and in
    the restatement), takes its second frame by map_add, and holds the restatement's map"""
    c = cases.full_plus_one()
    ego = state(c["constants"])
    with pytest.raises(RuntimeError, match=r"code -3\).*voxel table is full"):
        ego.register_frame(c["points"])
    ego.reset()
    assert ego.poses == [] and len(export(ego)[0]) == 0
    chain = made(cases.MAP_CASES, "chain_40")
    f0, f1 = chain["frames"][0][0], chain["frames"][1][0]
    odo = rest.Odometry()
    for f in (f0, f0):
        pose = ego.register_frame(f)
        assert np.array_equal(pose, odo.register_frame(f)) and np.array_equal(pose, np.eye(4))
    info = ego.frame_info()
    r = odo.records[1]
    assert (info["iterations"], info["correspondences"], info["frame_ds"], info["source"]) == \
        (r["iterations"], r["correspondences"], len(r["idx_ds"]), len(r["idx_source"]))
    ego.map_add(f1, np.eye(4))
    odo.map.update(f1, np.eye(4))
    assert_map(export(ego), odo.map.snapshot(), "after reset")
    assert max(len(v) for v in odo.map.cells.values()) == 3
    ego.close()


def test_coordinate_range_is_a_status_and_bad_rows_are_cropped():
    """voxel_size 1e-4: one point inside the crop beyond the 2^20 voxels of a key is ICPFLOW_E_LIMIT; the same frame without
    it passes; rows of NaN and +-inf raise nothing and are in neither list"""
    c = cases.coord_range()
    ego = state(c["constants"])
    with pytest.raises(RuntimeError, match=r"code -3\).*leaves the 2\^20 voxels"):
        ego.register_frame(np.concatenate([c["good"][:100], c["beyond"], c["good"][100:]]))
    ego.reset()
    assert np.array_equal(ego.register_frame(c["good"]), np.eye(4))
    assert ego.frame_info()["frame_ds"] == len(c["good"]) == ego.frame_info()["map_voxels"]
    ego.reset()
    frame = np.concatenate([c["good"][:50], c["bad"][:2], c["good"][50:], c["bad"][2:]])
    with np.errstate(invalid="ignore"):
        ds, src = rest.downsample(frame, 1.0, 100.0, 1e-4)
    got = [t.cpu().numpy() for t in ego.downsample(frame)]
    assert np.array_equal(got[0], ds) and np.array_equal(got[1], src) and len(ds) == len(c["good"])
    assert np.array_equal(ego.register_frame(frame), np.eye(4)) and ego.frame_info()["frame_ds"] == len(ds)
    ego.close()


def test_frame_path_equals_pieces():
    """three frames through register_frame (device-side counts, rows through the index lists), and through downsample +
    map_add with the poses the first run returned (host-side counts): the same map, order inside the voxels included, which
    is also the restatement's under those poses; frame_info counts what the lists and the export hold"""
    c = cases.three_frames()
    whole, pieces = state(c["constants"]), state(c["constants"])
    m = rest.VoxelMap(1.0, 20, 100.0)
    for j, f in enumerate(c["points"]):
        pose = whole.register_frame(f)
        info = whole.frame_info()
        ds, src = (t.cpu().numpy() for t in pieces.downsample(f))
        want_ds, want_src = rest.downsample(f, 1.0, 100.0, 1.0)
        assert np.array_equal(ds, want_ds) and np.array_equal(src, want_src)
        assert (info["frame_ds"], info["source"]) == (len(ds), len(src))
        pieces.map_add(f[ds], pose)
        m.update(f[want_ds], pose)
        a, b = export(whole), export(pieces)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), j
        assert info["map_voxels"] == len(a[0])
        assert_map(a, m.snapshot(), ("frame path", j))
        print(f"frame {j}: {info}")
        assert j == 0 or info["iterations"] >= 1
    whole.close()
    pieces.close()


# ============================================================================================ C: the down-sampling
@pytest.mark.parametrize("name", list(cases.DS_CASES))
def test_downsampling_equals_the_restatement(name):
    c = made(cases.DS_CASES, name)
    ego = state(c["constants"])
    with np.errstate(invalid="ignore"):
        ds, src = rest.downsample(c["points"], 1.0, 100.0, 1.0)
    got = run_downsample(ego, c)
    _first[name] = got
    print(f"{name}: {len(c['points'])} rows -> frame_ds {len(got[0])} / {len(ds)}, source {len(got[1])} / {len(src)}")
    assert np.array_equal(got[0], ds) and np.array_equal(got[1], src)
    ego.close()


# ============================================================================================ D: the registration
@pytest.mark.parametrize("name", list(cases.REG_CASES))
def test_registration_decisions(name):
    """register_step against a map put there with map_add: iterations and correspondences equal the restatement's, the pose
    is within POSE_BOUND of it; where no step is taken (fewer than 3 correspondences, dx = 0) the pose is the guess bit for
    bit"""
    c = made(cases.REG_CASES, name)
    ego = state(c["constants"])
    res = run_registration(ego, c)
    _first[name] = res
    check_registration(name, res, c["_want"], exact_pose=name in ("few[2]", "own_points", "m_seams[1]", "only_27[two away]"))
    if name == "cap_iterations[3]":
        assert int(res[16]) == 3 and res[17] > 1e-4
    ego.close()


def test_empty_source_and_pruned_map_on_both_paths():
    """include/icpflow_hip.h, 8(f) step 5: a source of no points, or a map whose voxels were all pruned, is one iteration that
    finds no correspondence and returns the guess -- through register_step (m = 0 known on the host) and through register_frame
    (a frame cropped to nothing; n = 0) alike, as the restatement says; 0 iterations only while the map has received nothing"""
    c = made(cases.REG_CASES, "own_points")
    g = cases.FEW_GUESS
    ego = state(c["constants"])
    res = ego.register_step(c["source"], g, 1.0).cpu().numpy()                        # nothing received yet
    assert np.array_equal(res[0:16].reshape(4, 4), g) and res[16:20].tolist() == [0.0, 0.0, 0.0, 0.0]
    ego.map_add(c["source"], np.eye(4))
    want = rest.register(np.zeros((0, 3), F), c["_map"].arrays(), g, 1.0, 1.0, fresh=False)
    assert want[1:] == (1, 0.0, 0)
    res = ego.register_step(np.zeros((0, 3), F), g, 1.0).cpu().numpy()                # m = 0
    assert np.array_equal(res[0:16].reshape(4, 4), want[0]) and res[16:20].tolist() == [1.0, 0.0, 0.0, 0.0]
    ego.map_add(np.zeros((0, 3), F), cases.translation(500.0, 0.0, 0.0))              # every voxel out of range
    assert len(export(ego)[0]) == 0
    res = ego.register_step(c["source"], g, 1.0).cpu().numpy()
    assert np.array_equal(res[0:16].reshape(4, 4), g) and res[16:20].tolist() == [1.0, 0.0, 0.0, 0.0]
    # ... and the frame path: frame 0, a frame cropped to nothing, a frame of no rows
    ego.reset()
    odo = rest.Odometry()
    for f in (c["source"], c["source"] * F(0.001), np.zeros((0, 3), F)):
        pose = ego.register_frame(f)
        assert np.array_equal(pose, odo.register_frame(f)) and np.array_equal(pose, np.eye(4))
        info, r = ego.frame_info(), odo.records[-1]
        assert (info["iterations"], info["correspondences"], info["frame_ds"], info["source"], info["final_dx"]) == \
            (r["iterations"], r["correspondences"], len(r["idx_ds"]), len(r["idx_source"]), r["final_dx"])
    assert [r["iterations"] for r in odo.records] == [0, 1, 1]
    assert_map(export(ego), odo.map.snapshot(), "after two empty frames")
    ego.close()


# ============================================================================================ E: independence
def _everything():
    return [(cases.MAP_CASES, n, run_map) for n in cases.MAP_CASES] + [(cases.DS_CASES, n, run_downsample) for n in cases.DS_CASES] + \
           [(cases.REG_CASES, n, run_registration) for n in cases.REG_CASES]


def _blob(out):
    if isinstance(out, np.ndarray):
        return out.tobytes()
    return b"|".join(_blob(o) for o in out)


def _baseline(table, name, run):
    if name not in _first:
        c = made(table, name)
        ego = state(c["constants"])
        _first[name] = run(ego, c)
        ego.close()
    return _blob(_first[name])


def test_rerun_after_reset_is_bit_identical():
    """every case of A - D twice on one state with reset() between: the slot a voxel lands in varies with arrival, and nothing
    that is read back may depend on it (nor on what the tables held before)"""
    total = 0
    for table, name, run in _everything():
        c = made(table, name)
        want = _baseline(table, name, run)
        ego = state(c["constants"])
        first = _blob(run(ego, c))
        ego.reset()
        second = _blob(run(ego, c))
        ego.close()
        assert first == want and second == want, name
        total += len(want)
    print(f"{len(_everything())} cases, {total} bytes of exports and results each time")


def test_second_state_on_a_second_stream():
    """two host threads, each with a stream and states of its own, run every case at the same time -- one from the first case
    to the last, one from the last to the first: bit-identical to the runs alone"""
    todo = _everything()
    want = {name: _baseline(table, name, run) for table, name, run in todo}
    got = {"a": {}, "b": {}}

    def worker(tag, order):
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):
            for table, name, run in order:
                c = made(table, name)
                ego = state(c["constants"])
                got[tag][name] = _blob(run(ego, c))
                ego.close()

    threads = [threading.Thread(target=worker, args=("a", todo)), threading.Thread(target=worker, args=("b", todo[::-1]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for tag in got:
        assert sorted(got[tag]) == sorted(want)
        assert [n for n in want if got[tag][n] != want[n]] == [], tag


def test_the_bound_leaves_no_room_for_a_wrong_decision():
    """(last in the file: reports the largest difference of this run.)  The bound is 4 x the largest measured difference and
    at least 10^6 below the margin every wrong decision has on the CPU (tests/test_ego_map_cases.py)"""
    print(f"largest GPU - restatement over this run: {_worst[0]:.3e} m {_worst[1]:.3e} rad; bound {POSE_BOUND_M:.3e} m {POSE_BOUND_RAD:.3e} rad")
    assert POSE_BOUND_M * 1e6 <= 1e-3 and POSE_BOUND_RAD * 1e6 <= 1e-4

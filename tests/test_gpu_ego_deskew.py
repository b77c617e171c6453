"""GPU: the ego-motion estimate's second configuration (include/icpflow_hip.h "8(f), second configuration": deskewing by
per-point stamps, a fixed threshold) against the fp64 restatement tests/ego_deskew_restatement.py and against truth, on the
inputs of tests/ego_deskew_scenes.py.  Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_deskew_restatement as dk     # noqa: E402
import ego_deskew_scenes as dscenes     # noqa: E402
import ego_motion_restatement as rest   # noqa: E402
import ego_motion_scenes as scenes      # noqa: E402

pytestmark = pytest.mark.gpu

# the bound tests/test_gpu_ego_motion.py asserts for one registration against the restatement's
STEP_BOUND_M, STEP_BOUND_RAD = 4 * 1.835e-15, 4 * 2.646e-17


def _ego(nmax, motion=None, **over):
    from icp_flow_amd import utils_ego_motion
    return utils_ego_motion.egomotion(None, "cuda:0", motion, max_points=nmax, map_capacity=1 << 16, **over)


def _map_of(ego):
    keys, counts, pts = (t.cpu().numpy() for t in ego.map_export())
    return {int(k): pts[v, : counts[v]] for v, k in enumerate(keys)}


def _same_map(got, want):
    if sorted(got) != sorted(want):
        return False
    srt = lambda a: a[np.lexsort(a.T[::-1])]   # noqa: E731
    return all(got[k].shape == want[k].shape and np.array_equal(srt(got[k]), srt(want[k])) for k in want)


# ---- the kernel alone --------------------------------------------------------------------------------------------------------
def test_kernel_within_one_float32_ulp_of_the_restatement():
    """Both sides evaluate exp((stamp - 0.5) xi) p in fp64 and round once to float32, so every coordinate is within one
    float32 ulp and at most 1e-4 of the coordinates are not bit-equal (tests/test_ego_deskew.py shows the inputs allow that:
    the restatement keeps it against itself with its sines off by 4 fp64 ulps).  A stamp that is not finite gives a row that
    is not finite, on both sides.

    Measured on the MI355X: 0 of 90006 finite coordinates not bit-equal, over the 7 twists x 5 sizes."""
    ego = _ego(max(dscenes.KERNEL_SIZES))
    total = differ = 0
    for name in dscenes.KERNEL_TWISTS:
        for n in dscenes.KERNEL_SIZES:
            points, stamps, poses = dscenes.kernel_case(name, n)
            got = ego.deskew(points, stamps, poses).cpu().numpy()
            want = dk.deskew(points, stamps, dk.se3_log(poses[1]))
            ok = np.isfinite(want)
            assert got.shape == (n, 3) and np.array_equal(ok, np.isfinite(got)), (name, n)
            assert np.array_equal(ok.all(axis=1), np.isfinite(stamps)) and np.array_equal(ok.any(axis=1), ok.all(axis=1))
            apart = dscenes.ulps_apart(got[ok], want[ok])
            print(f"{name} n={n}: {int((apart > 0).sum())} of {apart.size} coordinates not bit-equal, farthest {int(apart.max(initial=0))} ulp")
            assert apart.max(initial=0) <= 1, (name, n)
            total, differ = total + apart.size, differ + int((apart > 0).sum())
    print(f"all cases: {differ} of {total} coordinates not bit-equal")
    assert differ <= 1e-4 * total
    # the twists that move nothing: bit for bit the input
    points, stamps, poses = dscenes.kernel_case("zero", 4097)
    ok = np.isfinite(stamps)
    assert np.array_equal(ego.deskew(points, stamps, poses).cpu().numpy()[ok], points[ok])
    ego.close()


def test_fewer_than_two_poses_copy_and_a_nan_row_never_reaches_the_lists():
    points, stamps, poses = dscenes.kernel_case("turn", 4097)
    ego = _ego(4097)
    bad = np.nonzero(~np.isfinite(stamps))[0]
    assert len(bad) == 1
    for have in (0, 1):
        out = ego.deskew(points, stamps)                                   # the state's own poses: none, then one
        assert torch.equal(out.cpu().view(torch.int32), torch.from_numpy(points).view(torch.int32)), have
        ego.register_frame(points[:64], None)
        assert len(ego.poses) == have + 1
    out = ego.deskew(points, stamps, poses)
    assert not torch.isfinite(out[bad[0]]).any() and int((~torch.isfinite(out)).any(dim=1).sum()) == 1
    idx_ds, idx_source = (t.cpu().numpy() for t in ego.downsample(out))
    with np.errstate(invalid="ignore"):
        want_ds, want_source = rest.downsample(out.cpu().numpy(), 1.0, 100.0, ego.voxel_size)
    assert np.array_equal(idx_ds, want_ds) and np.array_equal(idx_source, want_source)
    assert len(idx_ds) > 1000 and bad[0] not in idx_ds and bad[0] not in idx_source
    ego.close()


# ---- off means off -------------------------------------------------------------------------------------------------------------
def test_off_is_the_old_call_bit_for_bit():
    """icpflow_egomotion_register_frame_stamped with deskew 0 (stamps given), and with deskew 1 but NULL stamps, d_corrected
    NULL both times: the poses, frame_info and the exported map of icpflow_ego_register_frame."""
    from icp_flow_amd import _lib
    frames, _ = scenes.exact_path(num_frames=4)
    frames = [np.ascontiguousarray(f[::3]) for f in frames]
    nmax = max(len(f) for f in frames)

    def run(mode):
        ego = _ego(nmax, None if mode != "null_stamps" else dict(deskew=True))
        poses, infos = [], []
        for j, f in enumerate(frames):
            if mode == "old":
                poses.append(ego.register_frame(f, None))
            else:
                pts = ego._points(f)
                stamps = torch.linspace(0, 1, len(f), device="cuda:0") if mode == "deskew_0" else None
                out = (ctypes.c_double * 16)()
                _lib.call("icpflow_egomotion_register_frame_stamped", ego._h, _lib.ptr(pts), _lib.ptr(stamps), len(f), None, out,
                          _lib.stream(ego.device))
                poses.append(np.array(out).reshape(4, 4))
            infos.append(ego.frame_info())
        exported = ego.map_export()
        ego.close()
        return np.stack(poses), infos, exported

    want = run("old")
    assert want[1][-1]["sigma"] != 10.0 and want[1][-1]["iterations"] > 0
    for mode in ("deskew_0", "null_stamps"):
        got = run(mode)
        assert np.array_equal(want[0].view(np.uint64), got[0].view(np.uint64)), mode
        assert want[1] == got[1], mode
        assert all(torch.equal(a, b) for a, b in zip(want[2], got[2])), mode


# ---- on ------------------------------------------------------------------------------------------------------------------------
def test_on_a_teacher_forced_frame():
    """Frame 2 of the skewed sequence: d_corrected is the piece's output; the restatement run on THAT output keeps the same
    rows in both down-samplings, its one registration (same source, map, guess, sigma) agrees within the step bound of
    tests/test_gpu_ego_motion.py, and the map after the frame is the same voxel by voxel.

    Measured on the MI355X: 0 of 12000 corrected coordinates not bit-equal to the restatement's deskewing under the GPU's own
    poses; the registration ends 1.731e-16 m / 1.999e-17 rad from the restatement's, 3 iterations and 1747 correspondences on
    both sides (the bound: 7.34e-15 m, 1.06e-16 rad)."""
    frames, stamps, _, _, _ = dscenes.skewed_runs()
    ego = _ego(len(frames[0]), dict(deskew=True))
    for j in (0, 1):
        ego.register_frame(frames[j], stamps[j])
        assert torch.equal(ego.corrected.cpu().view(torch.int32), torch.from_numpy(frames[j]).view(torch.int32))     # a copy: no twist yet
    piece = ego.deskew(frames[2], stamps[2])
    ego.register_frame(frames[2], stamps[2])
    assert torch.equal(ego.corrected, piece) and not np.array_equal(piece.cpu().numpy(), frames[2])
    corrected = ego.corrected.cpu().numpy()
    # ... which is the restatement's deskewing under the GPU's own two poses, to the kernel test's bound
    want = dk.deskew(frames[2], stamps[2], dk.se3_log(rest.rigid_inverse(ego.poses[0]) @ ego.poses[1]))
    apart = dscenes.ulps_apart(corrected, want)
    print(f"frame 2: {int((apart > 0).sum())} of {apart.size} corrected coordinates not bit-equal to the restatement's")
    assert apart.max() <= 1 and (apart > 0).sum() <= 1e-4 * apart.size
    ego.close()
    # the restatement: frames 0 and 1 as they are, then the GPU's corrected frame 2
    odo = dk.StampedOdometry()
    for f in (frames[0], frames[1], corrected):
        odo.register_frame(f)
    forced = _ego(len(frames[0]))
    for j in (0, 1):
        forced.map_add(frames[j][odo.records[j]["idx_ds"]], odo.records[j]["pose"])
    r = odo.records[2]
    idx_ds, idx_source = (t.cpu().numpy() for t in forced.downsample(corrected))
    assert np.array_equal(idx_ds, r["idx_ds"]) and np.array_equal(idx_source, r["idx_source"])
    res = forced.register_step(corrected[r["idx_source"]], r["guess"], r["sigma"]).cpu().numpy()
    dt, dth = rest.pose_error(res[0:16].reshape(4, 4), r["pose"])
    print(f"frame 2: GPU - restatement {dt:.3e} m {dth:.3e} rad; iterations {int(res[16])} / {r['iterations']}; "
          f"correspondences {int(res[18])} / {r['correspondences']}")
    assert int(res[16]) == r["iterations"] and int(res[18]) == r["correspondences"]
    assert dt < STEP_BOUND_M and dth < STEP_BOUND_RAD, (dt, dth)
    forced.map_add(corrected[r["idx_ds"]], r["pose"])
    assert _same_map(_map_of(forced), r["map"])
    forced.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _run_skewed(motion, via_estimate_poses=False):
    from icp_flow_amd import utils_ego_motion
    frames, stamps, _, _, _ = dscenes.skewed_runs()
    if via_estimate_poses:
        return utils_ego_motion.estimate_poses(frames, None, "cuda:0", timestamps=stamps, motion=motion, map_capacity=1 << 16)
    ego = _ego(len(frames[0]), motion)
    out = np.stack([ego.register_frame(f, s) for f, s in zip(frames, stamps)])
    ego.close()
    return out


def test_skewed_sequence_end_to_end():
    """A static world, a spinning sensor on a constant twist, every point seen from the pose of its stamp (the condition on
    the scene -- the restatement is at least twice as far from truth without deskewing -- is tests/test_ego_deskew.py's).
    With deskewing every pose is within the sequence bound of tests/test_gpu_ego_motion.py, |dt| + 50 m * dtheta < 0.1 m, of
    truth, and on every frame that is deskewed (2 ..) closer to truth than the GPU's own run without.

    Measured on the MI355X, |dt| + 50 m * dtheta per frame 0 .. 5 (the restatement's figures agree to the printed digits):
        with deskewing     0.0000  0.0043  0.0039  0.0032  0.0049  0.0031 m
        without            0.0000  0.0043  1.1075  1.1769  1.2482  1.3158 m"""
    _, _, truth, _, rest_on = dscenes.skewed_runs()
    on, off = _run_skewed(dict(deskew=True)), _run_skewed(None)
    for j in range(len(truth)):
        e_on, e_off = scenes.cap_expression(on[j], truth[j]), scenes.cap_expression(off[j], truth[j])
        print(f"skewed frame {j}: |dt| + 50 dtheta = {e_on:.4f} m with deskewing (restatement {scenes.cap_expression(rest_on.poses[j], truth[j]):.4f} m), "
              f"{e_off:.4f} m without")
        assert e_on < 0.1, (j, e_on)
        if j >= 2:
            assert e_on < e_off, (j, e_on, e_off)
        else:
            assert np.array_equal(on[j], off[j])
    # stamps with deskewing off are ignored; estimate_poses hands the stamps through
    assert np.array_equal(_run_skewed(dict(deskew=False)), off)
    assert np.array_equal(_run_skewed(dict(deskew=True), via_estimate_poses=True), on)


# ---- the fixed threshold -------------------------------------------------------------------------------------------------------
def test_fixed_threshold_is_sigma_on_every_frame():
    """sigma is the fixed value on every frame, also once the sensor has moved 5 min_motion_th from frame 0 and the adaptive
    threshold would have taken over; the poses are the restatement's (same setting) within the sequence bound.

    Measured on the MI355X: GPU - restatement at most 2.6e-14 m of |dt| + 50 m * dtheta over 4 frames; the adaptive run's
    sigma on the same frames: 10, 10, 2.193, 1.558."""
    frames, _ = scenes.exact_path(num_frames=4)
    frames = [np.ascontiguousarray(f[::2]) for f in frames]
    odo = dk.StampedOdometry(fixed_threshold=2.0)
    for f in frames:
        odo.register_frame(f, keep_map=False)
    ego, free = _ego(max(len(f) for f in frames), dict(fixed_threshold=2.0)), _ego(max(len(f) for f in frames))
    for j, f in enumerate(frames):
        pose = ego.register_frame(f, None)
        free.register_frame(f, None)
        cap = scenes.cap_expression(pose, odo.poses[j])
        print(f"fixed threshold, frame {j}: sigma {ego.frame_info()['sigma']} (adaptive run: {free.frame_info()['sigma']:.3f}); "
              f"GPU - restatement |dt| + 50 dtheta = {cap:.3e} m; moved {np.linalg.norm(pose[0:3, 3]):.2f} m")
        assert ego.frame_info()["sigma"] == 2.0 and cap < 0.1
    assert np.linalg.norm(pose[0:3, 3]) > 0.5 and free.frame_info()["sigma"] not in (2.0, 10.0)      # the adaptive one had taken over
    ego.reset()                                                                                       # the setting outlives a reset
    ego.register_frame(frames[0], None)
    assert ego.frame_info()["sigma"] == 2.0
    ego.close()
    free.close()


# ---- reruns, streams, rejection ------------------------------------------------------------------------------------------------
def test_reruns_and_two_states_on_two_streams_are_bit_identical():
    first, second = _run_skewed(dict(deskew=True)), _run_skewed(dict(deskew=True))
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64))
    fixed = _run_skewed(dict(deskew=True, fixed_threshold=3.0))
    got = {}

    def worker(name, motion):
        with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):
            got[name] = _run_skewed(motion)

    threads = [threading.Thread(target=worker, args=("a", dict(deskew=True))),
               threading.Thread(target=worker, args=("b", dict(deskew=True, fixed_threshold=3.0)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert np.array_equal(got["a"].view(np.uint64), first.view(np.uint64)) and np.array_equal(got["b"].view(np.uint64), fixed.view(np.uint64))


def test_on_with_stamps_and_no_room_for_the_corrected_frame_is_refused_with_nothing_written():
    from icp_flow_amd import _lib
    frames, stamps, _, _, _ = dscenes.skewed_runs()
    ego = _ego(len(frames[0]), dict(deskew=True))
    for j in (0, 1):
        ego.register_frame(frames[j], stamps[j])
    torch.cuda.synchronize()
    before, poses, info = ego._mem.clone(), ego.poses, ego.frame_info()
    pts, st = ego._points(frames[2]), ego._stamps(stamps[2], len(frames[2]))
    out = (ctypes.c_double * 16)(*([7.0] * 16))
    rc = _lib._L.icpflow_egomotion_register_frame_stamped(ego._h, _lib.ptr(pts), _lib.ptr(st), len(frames[2]), None, out, _lib.stream(ego.device))
    assert rc == -1 and b"null pointer" in _lib._L.icpflow_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ego._mem, before) and list(out) == [7.0] * 16 and ego.frame_info() == info
    assert len(ego.poses) == 2 and all(np.array_equal(a, b) for a, b in zip(ego.poses, poses))
    # the state goes on as if the call had not been made
    want = _run_skewed(dict(deskew=True))[2]
    assert np.array_equal(ego.register_frame(frames[2], stamps[2]), want)
    ego.close()


def test_sequence_file_with_point_time(tmp_path):
    """load_sequence(pose_source="estimate") hands a file's `point_time` key to the estimate only when args.ego_motion turns
    deskewing on: the poses of the two direct runs, bit for bit."""
    from icp_flow_amd import frame_pairs
    frames, stamps, truth, _, _ = dscenes.skewed_runs()
    os.makedirs(tmp_path / "val")
    path = str(tmp_path / "val" / "s0.npz")
    np.savez(path, raw_points=np.concatenate(frames), time_indice=np.concatenate([np.full(len(f), j) for j, f in enumerate(frames)]),
             point_time=np.concatenate(stamps), ego_motion_gt=truth)
    for motion in (dict(deskew=True), None, dict(fixed_threshold=3.0)):
        a = frame_pairs.default_args()
        if motion is not None:
            a.ego_motion = motion
        fps = frame_pairs.load_sequence(path, a, pose_source="estimate")
        want = _run_skewed(motion)
        assert [fp.pose_source for fp in fps] == ["estimate"] * (len(frames) - 1)
        assert all(np.array_equal(fp.pose_exact, want[j + 1]) for j, fp in enumerate(fps)), motion

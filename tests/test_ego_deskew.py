"""CPU-only: the ego-motion estimate's second configuration (include/icpflow_hip.h "8(f), second configuration": deskewing by
per-point stamps, a fixed threshold) is declared, exported and bound, its argument errors are status codes, callers without
stamps take the call they always took -- and the yardstick of the GPU tests, tests/ego_deskew_restatement.py, is checked
against itself, with the two conditions the GPU tests lean on: the bound of the kernel test, and the skewed scene."""
import contextlib
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_deskew_restatement as dk     # noqa: E402
import ego_deskew_scenes as dscenes     # noqa: E402
import ego_motion_restatement as rest   # noqa: E402
import ego_motion_scenes as scenes      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"icpflow_egomotion_default_params": 1, "icpflow_egomotion_set_params": 2, "icpflow_egomotion_deskew": 7,
           "icpflow_egomotion_register_frame_stamped": 7}


def test_exports_are_declared_exported_and_bound():
    import __graft_entry__ as entry
    lib = ctypes.CDLL(entry.build())
    from icp_flow_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "icpflow_hip.h")).read(), flags=re.S)
    declared = {name: len(args.split(",")) for name, args in re.findall(r"\b(icpflow_egomotion_[a-z_]+)\s*\(([^)]*)\)", hdr)}
    assert declared == EXPORTS
    for name, count in EXPORTS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == count, name
    assert _lib.SIGNATURES["icpflow_egomotion_deskew"][1][3] is ctypes.c_int                     # n
    assert _lib.SIGNATURES["icpflow_egomotion_register_frame_stamped"][1][3] is ctypes.c_int
    assert ctypes.sizeof(_lib.EgoMotionParams) == 32                                              # size_t, two ints, two doubles on LP64
    assert ctypes.sizeof(_lib.EgoParams) == 72                                                    # the first configuration keeps its layout


def test_defaults_are_off_middle_adaptive():
    from icp_flow_amd import _lib, utils_ego_motion
    p = _lib.EgoMotionParams.defaults()
    assert (p.struct_size, p.deskew, p.reserved, p.mid_stamp, p.fixed_threshold) == (32, 0, 0, 0.5, 0.0)
    assert utils_ego_motion.MOTION_DEFAULTS == dict(deskew=False, mid_stamp=0.5, fixed_threshold=0.0)
    assert utils_ego_motion.read_motion(None) == utils_ego_motion.MOTION_DEFAULTS
    args = SimpleNamespace(ego_motion=dict(deskew=True, fixed_threshold=2.0))
    assert utils_ego_motion.read_motion(args, dict(fixed_threshold=0.3)) == dict(deskew=True, mid_stamp=0.5, fixed_threshold=0.3)
    with pytest.raises(TypeError, match="unknown motion setting"):
        utils_ego_motion.read_motion(None, dict(voxel_size=1.0))
    with pytest.raises(TypeError, match="unknown motion setting"):
        utils_ego_motion.read_motion(SimpleNamespace(ego_motion=dict(deskewing=True)))
    with pytest.raises(TypeError, match="unknown constant"):                                      # the constants stay a mapping of their own
        utils_ego_motion.read_constants(None, deskew=True)


def test_argument_errors_are_status_codes_with_messages():
    from icp_flow_amd import _lib
    L, one = _lib._L, ctypes.c_void_p(256)      # (a handle that is never followed: every call below is refused before it would be)
    err = lambda: L.icpflow_last_error()   # noqa: E731
    assert L.icpflow_egomotion_default_params(None) == -1 and b"null pointer" in err()
    good = _lib.EgoMotionParams.defaults()
    assert L.icpflow_egomotion_set_params(None, ctypes.byref(good)) == -1 and b"null pointer" in err()
    assert L.icpflow_egomotion_set_params(one, None) == -1 and b"null pointer" in err()
    nan, inf = float("nan"), float("inf")
    for field, bad, word in (("struct_size", 24, b"struct_size"), ("deskew", 2, b"deskew"), ("mid_stamp", nan, b"mid_stamp"),
                             ("mid_stamp", inf, b"mid_stamp"), ("mid_stamp", -0.5, b"mid_stamp"), ("fixed_threshold", nan, b"fixed_threshold"),
                             ("fixed_threshold", inf, b"fixed_threshold"), ("fixed_threshold", -1.0, b"fixed_threshold")):
        q = _lib.EgoMotionParams.defaults(**{field: bad})
        assert L.icpflow_egomotion_set_params(one, ctypes.byref(q)) == -1 and word in err(), (field, bad)
    pose = (ctypes.c_double * 16)()
    assert L.icpflow_egomotion_deskew(None, one, one, 4, None, one, None) == -1 and b"null pointer" in err()
    assert L.icpflow_egomotion_register_frame_stamped(None, one, one, 4, one, pose, None) == -1 and b"null pointer" in err()


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_ego_motion
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            utils_ego_motion.egomotion(None, None, dict(deskew=True))
        with pytest.raises(RuntimeError, match="needs a GPU"):
            utils_ego_motion.estimate_poses([np.zeros((4, 3), np.float32)], timestamps=[np.zeros(4, np.float32)], motion=dict(deskew=True))
    with pytest.raises(ValueError, match="arrays of stamps"):
        utils_ego_motion.estimate_poses([np.zeros((4, 3), np.float32)] * 2, timestamps=[np.zeros(4, np.float32)])


def test_register_frame_without_per_point_stamps_takes_the_call_it_always_took(monkeypatch):
    from icp_flow_amd import _lib, utils_ego_motion
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, len(a))))
    monkeypatch.setattr(_lib, "stream", lambda dev: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    ego = object.__new__(utils_ego_motion.egomotion)            # (no device: the state is never created, only the dispatch runs)
    ego.device, ego._h, ego.corrected = torch.device("cpu"), None, None
    frame = np.arange(30, dtype=np.float32).reshape(10, 3)
    per_point = np.linspace(0, 1, 10, dtype=np.float32)
    old, new = ("icpflow_ego_register_frame", 5), ("icpflow_egomotion_register_frame_stamped", 7)
    ego.motion = dict(utils_ego_motion.MOTION_DEFAULTS, deskew=True)
    for stamps in (None, 0.5, np.float32(0.3), np.array(0.7), torch.tensor(0.5)):
        ego.register_frame(frame, stamps)
        assert calls.pop() == old and ego.corrected is None, stamps
    for stamps in (per_point, per_point.tolist(), torch.from_numpy(per_point)):
        ego.register_frame(frame, stamps)
        assert calls.pop() == new and tuple(ego.corrected.shape) == (10, 3)
    with pytest.raises(RuntimeError, match="expected 10 stamps"):
        ego.register_frame(frame, per_point[:9])
    ego.motion = dict(utils_ego_motion.MOTION_DEFAULTS)                                           # off: an array is ignored, as before
    for stamps in (None, 0.5, per_point, per_point[:9]):
        ego.register_frame(frame, stamps)
        assert calls.pop() == old and ego.corrected is None
    assert calls == []


def test_command_line_has_the_two_switches():
    import io
    from icp_flow_amd import frame_pairs
    buf = io.StringIO()
    with pytest.raises(SystemExit), contextlib.redirect_stdout(buf):
        frame_pairs.main(["--help"])
    assert "--ego-deskew" in buf.getvalue() and "--ego-fixed-threshold" in buf.getvalue()


# ---- the yardstick against itself ----------------------------------------------------------------------------------------------
def _scene_poses():
    out = [scenes.rigid(1.2, 0.3, 1.5)]
    for truth in (scenes.exact_path()[1], scenes.synthetic_static(n_points=50)[1], dscenes.skewed_sequence(n_points=50)[2]):
        out += list(truth) + [rest.rigid_inverse(a) @ b for a, b in zip(truth[:-1], truth[1:])]
    return out


def test_restatement_exp_of_log_is_the_pose():
    poses = _scene_poses()
    assert len(poses) > 20
    for T in poses:
        assert np.abs(dk.se3_exp(dk.se3_log(T)) - T).max() <= 1e-14
    for name, xi in dscenes.KERNEL_TWISTS.items():           # and log of exp is the twist (1e-3 short of a half turn the axis is
        back = dk.se3_log(dk.se3_exp(xi))                    # read off a skew part of 1e-3: three digits fewer)
        assert np.abs(back - xi).max() <= (1e-11 if name == "half_turn_nearly" else 1e-14), name


def test_restatement_exp_is_the_power_series():
    """40 terms of sum M^k / k! of the 4 x 4 twist matrix; bound: 40 terms, each partial sum below e^|M|, fp64 rounding"""
    rng = np.random.default_rng(5)
    twists = list(dscenes.KERNEL_TWISTS.values()) + [np.concatenate([rng.normal(0, 2, 3), a * rng.normal(0, 1, 3)]) for a in (1e-6, 1e-3, 0.1, 1.0)]
    for xi in twists + [0.5 * xi for xi in twists]:
        M, term, total = rest.twist_matrix(xi), np.eye(4), np.eye(4)
        for k in range(1, 41):
            term = term @ M / k
            total = total + term
        bound = 40 * np.exp(np.linalg.norm(M)) * np.finfo(np.float64).eps
        assert np.abs(dk.se3_exp(xi) - total).max() <= bound, (xi, bound)


def test_restatement_deskew_is_exp_of_the_scaled_twist_per_point():
    for name in ("translation", "switch_restatement", "turn", "half_turn_nearly"):
        points, stamps, poses = dscenes.kernel_case(name, 65)
        xi = dk.se3_log(poses[1])
        got = dk.deskew(points, stamps, xi)
        for i in range(len(points)):
            if not np.isfinite(stamps[i]):
                assert not np.isfinite(got[i]).any()
                continue
            T = dk.se3_exp((np.float64(stamps[i]) - 0.5) * xi)
            want = (T[0:3, 0:3] @ points[i].astype(np.float64) + T[0:3, 3]).astype(np.float32)
            assert dscenes.ulps_apart(got[i], want).max() <= 1, (name, i)
    assert np.array_equal(dk.deskew(points, np.full(65, 0.5, np.float32), xi), points)          # the middle of the sweep stays


def test_kernel_bound_holds_between_two_fp64_evaluations():
    """The bound of the GPU kernel test -- every coordinate within one float32 ulp, at most 1e-4 of them not bit-equal -- is a
    condition on its inputs: it holds here between the restatement and the restatement with every sine off by 4 fp64 ulps, up
    and down (two fp64 evaluations differ by a few ulps of their sincos; the restatement's coefficients take no cosine: it has
    1 - cos t as 2 sin^2(t / 2)), on the very inputs of the GPU test."""
    eps = np.finfo(np.float64).eps
    total = differ = 0
    for name in dscenes.KERNEL_TWISTS:
        for n in dscenes.KERNEL_SIZES:
            points, stamps, poses = dscenes.kernel_case(name, n)
            xi = dk.se3_log(poses[1])
            want = dk.deskew(points, stamps, xi)
            for sign in (1.0, -1.0):
                got = dk.deskew(points, stamps, xi, sin=lambda t: np.sin(t) * (1.0 + sign * 4 * eps))
                ok = np.isfinite(want)
                assert np.array_equal(ok, np.isfinite(got)) and np.array_equal(ok.all(axis=1), np.isfinite(stamps))
                apart = dscenes.ulps_apart(got[ok], want[ok])
                assert apart.max(initial=0) <= 1, (name, n)
                total, differ = total + apart.size, differ + int((apart > 0).sum())
    print(f"perturbed by 4 ulps: {differ} of {total} coordinates not bit-equal")
    assert differ <= 1e-4 * total
    seen = np.concatenate([dscenes.kernel_case("turn", n)[1] for n in dscenes.KERNEL_SIZES])
    assert all((seen == s).any() for s in dscenes.SPECIAL_STAMPS[:-1]) and np.isnan(seen).any()


def test_skewed_scene_needs_deskewing():
    """The condition on the scene of the GPU's end-to-end test: the restatement's pose error (|dt| + 50 m * dtheta) without
    deskewing is at least twice its error with it -- on every frame that is deskewed (2 ..) and so on their sum -- and with it
    the poses are within the sequence bound of 0.1 m of truth."""
    frames, stamps, truth, off, on = dscenes.skewed_runs()
    assert len(frames) == 6 and all(len(f) == 4000 for f in frames)
    assert all((s == 0.5).all() for s in stamps[:2]) and all(s.min() < 0.01 and s.max() > 0.99 for s in stamps[2:])
    for j in range(len(frames)):
        e_off, e_on = scenes.cap_expression(off.poses[j], truth[j]), scenes.cap_expression(on.poses[j], truth[j])
        print(f"skewed frame {j}: |dt| + 50 dtheta = {e_off:.4f} m without deskewing, {e_on:.4f} m with")
        assert e_on < 0.1
        if j >= 2:
            assert e_off >= 2.0 * e_on, (j, e_off, e_on)
        else:
            assert np.array_equal(off.poses[j], on.poses[j])
    assert "corrected" in on.records[2] and not np.array_equal(on.records[2]["corrected"], frames[2])


def test_restatement_fixed_threshold_replaces_sigma_only():
    frames, _ = scenes.exact_path(num_frames=3)
    frames = [f[::4] for f in frames]
    fixed, adaptive = dk.StampedOdometry(fixed_threshold=2.0), dk.StampedOdometry()
    for f in frames:
        fixed.register_frame(f, keep_map=False)
        adaptive.register_frame(f, keep_map=False)
    assert [r["sigma"] for r in fixed.records] == [2.0] * 3 and adaptive.records[1]["sigma"] == 10.0
    assert fixed.samples == adaptive.samples > 0                     # step 6 keeps its books

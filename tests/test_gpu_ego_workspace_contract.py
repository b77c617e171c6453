"""The ego-motion state's memory contract, in the style of tests/test_gpu_workspace_contract.py: "the caller owns the memory".
The state runs on EXACTLY icpflow_ego_state_bytes() bytes, filled with a poison, between two guards in the same
allocation, its outputs between guards as well; asserted: status 0, every guard byte intact, every output bit-identical
to an ordinary run, and one byte too few refused with ICPFLOW_E_WORKSPACE before anything is written.

Who initialises what (csrc/ego.hip): the live map table's keys and counts, flags, counts: hipMemsetAsync in create / reset;
the other table's keys and counts: hipMemsetAsync before every prune; a voxel's points: written below the count that
admits them; the scratch table: two memsets per down-sampling; slotOf, moved, sameTotal, idx lists: written for every row
below the count that bounds their readers; result: the registration (or the guess kernel) before map_add reads it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_motion_scenes as scenes      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
GUARD_BYTE = 0x5C


def _guarded(nbytes, poison, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _run(frames, dev, poison=None):
    """-> (poses, per frame idx_ds / idx_source / counts, exported map); guarded and poisoned when `poison` is given"""
    from icp_flow_amd import _lib
    L = _lib._L
    nmax = max(len(f) for f in frames)
    par = _lib.EgoParams.defaults(max_points=nmax, map_capacity=1 << 14)
    need = L.icpflow_ego_state_bytes(ctypes.byref(par))
    st = _lib.stream(dev)
    cap = 4096
    sizes = dict(mem=need, idx_ds=4 * nmax, idx_src=4 * nmax, counts=8, keys=8 * cap, mcounts=4 * cap, pts=4 * 60 * cap, num=4)
    if poison is None:
        bufs = {k: torch.zeros(v, dtype=torch.uint8, device=dev) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison, dev) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
        # one byte too few: refused before anything is written
        h = ctypes.c_void_p()
        before = bufs["mem"].clone()
        assert L.icpflow_ego_create(ctypes.byref(par), ctypes.c_void_p(at["mem"]), need - 1, st, ctypes.byref(h)) == -2
        torch.cuda.synchronize()
        assert not h.value and torch.equal(bufs["mem"], before)
    view = lambda k: (bufs[k] if poison is None else bufs[k][GUARD: GUARD + sizes[k]])   # noqa: E731
    h = ctypes.c_void_p()
    _lib.call("icpflow_ego_create", ctypes.byref(par), ctypes.c_void_p(at["mem"]), need, st, ctypes.byref(h))
    poses, lists = [], []
    for f in frames:
        pts = torch.from_numpy(f).to(dev)
        n = len(f)
        _lib.call("icpflow_ego_downsample", h, _lib.ptr(pts), n, ctypes.c_void_p(at["idx_ds"]), ctypes.c_void_p(at["idx_src"]),
                  ctypes.c_void_p(at["counts"]), st)
        c = view("counts").view(torch.int32).tolist()
        lists.append((c, view("idx_ds").view(torch.int32)[: c[0]].clone(), view("idx_src").view(torch.int32)[: c[1]].clone()))
        out = (ctypes.c_double * 16)()
        _lib.call("icpflow_ego_register_frame", h, _lib.ptr(pts), n, out, st)
        poses.append(np.array(out))
    _lib.call("icpflow_ego_map_export", h, ctypes.c_void_p(at["keys"]), ctypes.c_void_p(at["mcounts"]), ctypes.c_void_p(at["pts"]), cap,
              ctypes.c_void_p(at["num"]), st)
    torch.cuda.synchronize()
    v = int(view("num").view(torch.int32)[0])
    assert 0 < v <= cap
    keys = view("keys").view(torch.int64)[:v]
    order = torch.argsort(keys)
    exported = (keys[order].clone(), view("mcounts").view(torch.int32)[:v][order].clone(), view("pts").view(torch.float32).reshape(cap, 60)[:v][order].clone())
    L.icpflow_ego_destroy(h)
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
    return np.stack(poses), lists, exported


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_state_runs_on_exactly_its_bytes_whatever_they_held(poison):
    dev = torch.device("cuda:0")
    frames, _ = scenes.exact_path(num_frames=3)
    frames = [f[::4].copy() for f in frames]
    want = _run(frames, dev)
    got = _run(frames, dev, poison)
    assert np.array_equal(want[0].view(np.uint64), got[0].view(np.uint64))
    for (c0, a0, b0), (c1, a1, b1) in zip(want[1], got[1]):
        assert c0 == c1 and torch.equal(a0, a1) and torch.equal(b0, b1)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(want[2], got[2]))


def test_limits_are_status_codes():
    from icp_flow_amd import _lib
    L, dev = _lib._L, torch.device("cuda:0")
    par = _lib.EgoParams.defaults(max_points=1000, map_capacity=1024)
    need = L.icpflow_ego_state_bytes(ctypes.byref(par))
    mem = torch.empty(need, dtype=torch.uint8, device=dev)
    h, out = ctypes.c_void_p(), (ctypes.c_double * 16)()
    _lib.call("icpflow_ego_create", ctypes.byref(par), _lib.ptr(mem), need, _lib.stream(dev), ctypes.byref(h))
    pts = torch.zeros((2000, 3), dtype=torch.float32, device=dev)
    assert L.icpflow_ego_register_frame(h, _lib.ptr(pts), 2000, out, _lib.stream(dev)) == -3 and b"max_points" in L.icpflow_last_error()
    # a map table that cannot hold the frame's voxels: refused after the frame, by name
    rng = np.random.default_rng(0)
    wide = torch.from_numpy(rng.uniform(-60, 60, size=(1000, 3)).astype(np.float32)).to(dev)
    rc = L.icpflow_ego_register_frame(h, _lib.ptr(wide), 1000, out, _lib.stream(dev))
    assert rc == 0 or (rc == -3 and b"table is full" in L.icpflow_last_error())
    L.icpflow_ego_destroy(h)

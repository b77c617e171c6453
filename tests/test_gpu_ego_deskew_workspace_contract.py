"""The memory contract of the deskewing calls, in the style of tests/test_gpu_ego_workspace_contract.py: "the caller owns the
memory".  d_out of icpflow_egomotion_deskew and d_corrected of icpflow_egomotion_register_frame_stamped are EXACTLY n * 3
floats, filled with a poison, between two guards in the same allocation; the state is exactly icpflow_ego_state_bytes()
bytes (its pinned size: the corrected frame lives in the caller's buffer, not in the state), poisoned and guarded too.
Asserted: status 0, every guard byte intact, every output bit-identical to an ordinary run.

Who writes what (csrc/ego.hip): ego_deskew_kernel writes rows 0 .. n-1 of its output, one thread per row, `i >= n` returns;
with fewer than two poses the output is a device-to-device copy of n * 12 bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ego_deskew_scenes as dscenes     # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
GUARD_BYTE = 0x5C


def _guarded(nbytes, poison, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _run(frames, stamps, dev, poison=None):
    """-> (poses, per frame the piece's output and d_corrected); guarded and poisoned when `poison` is given"""
    from icp_flow_amd import _lib
    L = _lib._L
    n = len(frames[0])
    assert all(len(f) == n for f in frames)
    par = _lib.EgoParams.defaults(max_points=n, map_capacity=1 << 14)
    need = L.icpflow_ego_state_bytes(ctypes.byref(par))
    st = _lib.stream(dev)
    sizes = dict(mem=need, out=12 * n, corrected=12 * n)
    if poison is None:
        bufs = {k: torch.zeros(v, dtype=torch.uint8, device=dev) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison, dev) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    view = lambda k: (bufs[k] if poison is None else bufs[k][GUARD: GUARD + sizes[k]]).view(torch.float32).reshape(n, 3)   # noqa: E731
    h = ctypes.c_void_p()
    _lib.call("icpflow_ego_create", ctypes.byref(par), ctypes.c_void_p(at["mem"]), need, st, ctypes.byref(h))
    motion = _lib.EgoMotionParams.defaults(deskew=1)
    _lib.call("icpflow_egomotion_set_params", h, ctypes.byref(motion))
    poses, outs = [], []
    for f, s in zip(frames, stamps):
        pts, sts = torch.from_numpy(f).to(dev), torch.from_numpy(s).to(dev)
        _lib.call("icpflow_egomotion_deskew", h, _lib.ptr(pts), _lib.ptr(sts), n, None, ctypes.c_void_p(at["out"]), st)
        out = (ctypes.c_double * 16)()
        _lib.call("icpflow_egomotion_register_frame_stamped", h, _lib.ptr(pts), _lib.ptr(sts), n, ctypes.c_void_p(at["corrected"]), out, st)
        torch.cuda.synchronize()
        poses.append(np.array(out))
        outs.append((view("out").clone(), view("corrected").clone()))
    L.icpflow_ego_destroy(h)
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
    return np.stack(poses), outs


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_deskewing_runs_on_exactly_its_bytes_whatever_they_held(poison):
    dev = torch.device("cuda:0")
    frames, stamps, _ = dscenes.skewed_sequence(num_frames=4, n_points=1001)
    assert 1001 % 256 != 0 and 1001 > 256                    # more than one block, a ragged last one
    want = _run(frames, stamps, dev)
    got = _run(frames, stamps, dev, poison)
    assert np.array_equal(want[0].view(np.uint64), got[0].view(np.uint64))
    for j, ((o0, c0), (o1, c1)) in enumerate(zip(want[1], got[1])):
        assert torch.equal(o0.view(torch.int32), o1.view(torch.int32)) and torch.equal(c0.view(torch.int32), c1.view(torch.int32)), j
        assert torch.equal(o0.view(torch.int32), c0.view(torch.int32)), j          # d_corrected is the piece's output
    moved = [not torch.equal(c.cpu(), torch.from_numpy(f)) for (_, c), f in zip(want[1], frames)]
    assert moved == [False, False, True, True]                # copies until two poses exist, then the kernel

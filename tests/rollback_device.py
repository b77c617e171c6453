"""What the GPU tests of the roll-back share, in the manner of tests/match_eval_device.py: the raw calls of icpflow_apply_icp,
icpflow_icp, icpflow_estimate_init_pose and icpflow_hist_icp on buffers the test owns -- a workspace of EXACTLY the size the library
asks for, filled with 0xFF (NaN floats, -1 integers), between two guards, and every output between two guards in an allocation of
its own, poisoned beforehand -- and the form in which d_T_out IS d_init (the header allows it).  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd             # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, OUT_POISON = 0xFF, 0xA5
POISON_WORD = np.uint32(0xA5A5A5A5)     # an ordinary negative float32, -2.87e-16, and no iteration count


def _at(buf):
    return ctypes.c_void_p(buf.data_ptr() + GUARD)


def _words(buf, nbytes, dtype, shape, name, written=True):
    assert rd._guards_intact(buf, nbytes), f"guard of {name} changed"
    w = buf[GUARD: GUARD + nbytes].clone().view(torch.int32).cpu().numpy()
    if written:
        assert not (w.view(np.uint32) == POISON_WORD).any(), f"{name}: words left unwritten"
    return w.view(dtype).reshape(shape)


class _Call:
    """the workspace of one call and its outputs; `done` checks the status, the guards and that every output word was written"""

    def __init__(self, B, N, lens=(0, 0, 0), **outputs):
        from icp_flow_amd import _lib
        self.lib, self.need = _lib, _lib.workspace_bytes(B, N, lens)
        self.ws = rd._guarded(self.need, WS_POISON)
        self.spec = outputs                                   # name -> (dtype, shape)
        self.bufs = {k: rd._guarded(int(np.prod(s)) * 4, OUT_POISON) for k, (_, s) in outputs.items()}

    def done(self, rc):
        msg = self.lib._L.icpflow_last_error().decode() if rc else ""
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:      # a fault on the device: nothing more is started on it in this session
            import pytest
            pytest.exit(f"the device reported an error after a call: {e}", returncode=3)
        assert rc == 0, (rc, msg)
        assert rd._guards_intact(self.ws, self.need), "guard of the workspace changed"
        return {k: _words(self.bufs[k], int(np.prod(s)) * 4, dt, s, k) for k, (dt, s) in self.spec.items()}


def _opts(lib, search=None, arith=None, flags=()):
    return lib.options(search=search, arith=arith, **{f: True for f in flags})


def apply_icp(S, D, init, thres=0.1, max_iterations=50, rel=1e-6, stop_mode=0, alias=False, stream=None, search=None, arith=None,
              flags=()):
    """One call of icpflow_apply_icp -> (T_out float32 [B, 4, 4], iterations).  alias: d_T_out is d_init, between its own guards."""
    s, d = upload(S, F), upload(D, F)
    B, N = int(s.shape[0]), int(s.shape[1])
    c = _Call(B, N, T=(F, (B, 4, 4)), iters=(np.int32, (1,)))
    L, ptr = c.lib._L, c.lib.ptr
    if alias:
        c.bufs["T"][GUARD: GUARD + B * 64] = torch.from_numpy(np.ascontiguousarray(init, F).view(np.uint8).reshape(-1)).to(DEV)
        pin = _at(c.bufs["T"])
    else:
        keep = upload(init, F)
        pin = ptr(keep)
    torch.cuda.synchronize()                                # (the uploads and the poison ran on the default stream)
    with _opts(c.lib, search, arith, flags), torch.cuda.stream(stream):
        rc = L.icpflow_apply_icp(ptr(s), ptr(d), pin, B, N, float(thres), int(max_iterations), float(rel), int(stop_mode),
                                 _at(c.bufs["T"]), _at(c.bufs["iters"]), _at(c.ws), c.need, c.lib.stream(DEV), c.lib.opt())
    out = c.done(rc)
    if not alias:
        assert np.array_equal(keep.cpu().numpy().view(np.uint32), np.ascontiguousarray(init, F).view(np.uint32)), "d_init was written"
    return out["T"], int(out["iters"][0])


def icp(X, Y, pre_pose, thres=0.1, max_iterations=50, rel=1e-6, stop_mode=0, stream=None, search=None, arith=None, flags=()):
    """One call of icpflow_icp -> (R [B, 3, 3], T [B, 3], iterations): the ICP of icpflow_apply_icp from the same initial poses"""
    x, y, pre = upload(X, F), upload(Y, F), upload(pre_pose, F)
    B, N = int(x.shape[0]), int(x.shape[1])
    c = _Call(B, N, R=(F, (B, 3, 3)), T=(F, (B, 3)), iters=(np.int32, (1,)))
    L, ptr = c.lib._L, c.lib.ptr
    torch.cuda.synchronize()
    with _opts(c.lib, search, arith, flags), torch.cuda.stream(stream):
        rc = L.icpflow_icp(ptr(x), ptr(y), ptr(pre), B, N, float(thres), int(max_iterations), float(rel), int(stop_mode), _at(c.bufs["R"]),
                           _at(c.bufs["T"]), None, _at(c.bufs["iters"]), None, _at(c.ws), c.need, c.lib.stream(DEV), c.lib.opt())
    out = c.done(rc)
    return out["R"], out["T"], int(out["iters"][0])


def _edges(thres, frame):
    from types import SimpleNamespace
    from icp_flow_amd import utils_hist
    ex, ey, ez = utils_hist.bin_edges(SimpleNamespace(thres_dist=thres, translation_frame=frame), DEV)
    return (ex, ey, ez), (len(ex), len(ey), len(ez)), float(thres // 2)


def estimate_init_pose(S, D, thres=0.1, frame=2.0, stream=None, flags=()):
    """One call of icpflow_estimate_init_pose -> T float32 [B, 4, 4]"""
    s, d = upload(S, F), upload(D, F)
    B, N = int(s.shape[0]), int(s.shape[1])
    (ex, ey, ez), lens, shift = _edges(thres, frame)
    c = _Call(B, N, lens, T=(F, (B, 4, 4)))
    L, ptr = c.lib._L, c.lib.ptr
    torch.cuda.synchronize()
    with _opts(c.lib, flags=flags), torch.cuda.stream(stream):
        rc = L.icpflow_estimate_init_pose(ptr(s), ptr(d), B, N, ptr(ex), lens[0], ptr(ey), lens[1], ptr(ez), lens[2], shift,
                                          _at(c.bufs["T"]), _at(c.ws), c.need, c.lib.stream(DEV), c.lib.opt())
    return c.done(rc)["T"]


def hist_icp(S, D, thres=0.1, frame=2.0, max_iterations=50, rel=1e-6, stop_mode=0, stream=None, flags=()):
    """One call of icpflow_hist_icp -> (T_out float32 [B, 4, 4], iterations)"""
    s, d = upload(S, F), upload(D, F)
    B, N = int(s.shape[0]), int(s.shape[1])
    (ex, ey, ez), lens, shift = _edges(thres, frame)
    c = _Call(B, N, lens, T=(F, (B, 4, 4)), iters=(np.int32, (1,)))
    L, ptr = c.lib._L, c.lib.ptr
    torch.cuda.synchronize()
    with _opts(c.lib, flags=flags), torch.cuda.stream(stream):
        rc = L.icpflow_hist_icp(ptr(s), ptr(d), B, N, ptr(ex), lens[0], ptr(ey), lens[1], ptr(ez), lens[2], shift, float(thres),
                                int(max_iterations), float(rel), int(stop_mode), _at(c.bufs["T"]), _at(c.bufs["iters"]), _at(c.ws),
                                c.need, c.lib.stream(DEV), c.lib.opt())
    out = c.done(rc)
    return out["T"], int(out["iters"][0])

"""The memory contract of icpflow_ground_segment, in the style of tests/test_gpu_seqeval_workspace_contract.py: "the caller
owns the memory".  It runs on EXACTLY its icpflow_ground_workspace_bytes() bytes, filled with a poison, between two guards in
the same allocation, at base + 16, its outputs between guards as well; asserted: the exact size, status 0, every guard byte
intact, labels and table bit-identical to an ordinary run, and one byte too few refused with ICPFLOW_E_WORKSPACE before
anything is written.

Who initialises what (csrc/ground.hip): the binning writes a patch id and a label for every row and every wave's count of
every patch; the scan writes all 505 starts; the scatter fills the places [0, start[504]) and nothing reads beyond them; a
patch's workgroup clears the states of its own points before it reads them and writes its whole table row."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_scenes as gs      # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 1 << 16
GUARD_BYTE = 0x5C
DEV = torch.device("cuda:0")


def _guarded(nbytes, poison):
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    buf[GUARD: GUARD + nbytes] = poison
    return buf


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + nbytes:] == GUARD_BYTE).all())


def _r256(b):
    return -(-b // 256) * 256


def _run(pts, poison=None):
    from icp_flow_amd import _lib
    L, st = _lib._L, _lib.stream(DEV)
    n = len(pts)
    x = torch.from_numpy(pts).to(DEV)
    par = _lib.GroundParams.defaults()
    need = L.icpflow_ground_workspace_bytes(n, ctypes.byref(par))
    waves = min(max(-(-n // 512), 1), 1024)
    assert need == 2 * _r256(4 * n) + _r256(12 * n) + _r256(n) + _r256(waves * 504 * 4) + _r256(505 * 4) + _r256(504 * 16 * 8)
    sizes = dict(ws=need, labels=n, table=504 * 16 * 8)
    if poison is None:
        bufs = {k: torch.zeros(v + 16, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
        at = {k: b.data_ptr() for k, b in bufs.items()}
    else:
        bufs = {k: _guarded(v, poison) for k, v in sizes.items()}
        at = {k: b.data_ptr() + GUARD for k, b in bufs.items()}
    args = lambda nbytes: (_lib.ptr(x), 3, n, ctypes.byref(par), ctypes.c_void_p(at["labels"]), ctypes.c_void_p(at["table"]),   # noqa: E731
                           ctypes.c_void_p(at["ws"]), ctypes.c_size_t(nbytes), st)
    if poison is not None:
        before = {k: b.clone() for k, b in bufs.items()}
        assert L.icpflow_ground_segment(*args(need - 1)) == -2 and b"workspace" in L.icpflow_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[k], before[k]) for k in bufs)
    _lib.call("icpflow_ground_segment", *args(need))
    torch.cuda.synchronize()
    if poison is not None:
        for k, b in bufs.items():
            assert _guards_intact(b, sizes[k]), f"guard of {k} changed (poison {poison:#x})"
        return tuple(bufs[k][GUARD: GUARD + sizes[k]].clone() for k in ("labels", "table"))
    return tuple(bufs[k][:sizes[k]].clone() for k in ("labels", "table"))


def _run_offset(pts):
    """the workspace at base + 16: 8-byte aligned is all the entry point asks for"""
    from icp_flow_amd import _lib
    L, n = _lib._L, len(pts)
    x = torch.from_numpy(pts).to(DEV)
    par = _lib.GroundParams.defaults()
    need = L.icpflow_ground_workspace_bytes(n, ctypes.byref(par))
    ws = _guarded(need + 16, 0xA5)
    labels = torch.zeros(n, dtype=torch.uint8, device=DEV)
    table = torch.zeros(504 * 16, dtype=torch.float64, device=DEV)
    _lib.call("icpflow_ground_segment", _lib.ptr(x), 3, n, ctypes.byref(par), _lib.ptr(labels), _lib.ptr(table),
              ctypes.c_void_p(ws.data_ptr() + GUARD + 16), ctypes.c_size_t(need), _lib.stream(DEV))
    torch.cuda.synchronize()
    assert _guards_intact(ws, need + 16) and bool((ws[GUARD: GUARD + 16] == 0xA5).all())
    return labels, table.view(torch.uint8)


@pytest.mark.parametrize("name", ["edges", "big_patch", "frame"])
def test_runs_on_exactly_its_bytes_whatever_they_held(name):
    pts, _ = gs.ALL[name]()
    want = _run(pts)
    for poison in (0x00, 0xA5, 0xFF):
        got = _run(pts, poison)
        assert all(torch.equal(a, b) for a, b in zip(want, got)), hex(poison)
    got = _run_offset(pts)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert int(want[0].sum()) < len(pts)

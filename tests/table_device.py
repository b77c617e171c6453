"""Device helper of tests/test_gpu_tables.py: raw C-ABI calls of icpflow_cluster_table, icpflow_cluster_table_pair and
icpflow_cluster_stats the way a C caller makes them -- the workspace EXACTLY *_workspace_bytes() bytes, filled with 0xFF, and the
workspace and every output between guards in one allocation (the harness of tests/test_gpu_workspace_contract.py restated
small: one allocation and one transfer per call).  A guard is 64 KiB: larger than every stride inside the carve (a row of `counts`
is Lmax * 4 <= 16 KiB) and than a table row; a condition, not a measurement.  Outputs are pre-filled with 0xFF too, so that a word
nobody wrote still reads as poison (-1 as an integer, a NaN as a float)."""
import contextlib
import ctypes
import time
from types import SimpleNamespace

import numpy as np
import torch

from icp_flow_amd import _lib

DEV = torch.device("cuda:0")
GUARD = 64 << 10
GUARD_BYTE = 0x3C
POISON = 0xFF
COLS = 9


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


class Arena:
    """[guard | region | guard | region | ... | guard], every region 256-byte aligned and filled with the poison"""

    def __init__(self, sizes):
        self.off, at = [], GUARD
        for n in sizes:
            self.off.append((at, int(n)))
            at = (at + int(n) + 255) // 256 * 256 + GUARD
        self.raw = torch.empty(at + 256, dtype=torch.uint8, device=DEV)
        self.shift = (-self.raw.data_ptr()) % 256
        self.raw.fill_(GUARD_BYTE)
        for o, n in self.off:
            self.raw[self.shift + o:self.shift + o + n].fill_(POISON)

    def ptr(self, k):
        return ctypes.c_void_p(self.raw.data_ptr() + self.shift + self.off[k][0])

    def fetch(self):
        """-> the regions as NumPy byte arrays, after every guard byte has been shown intact"""
        host = self.raw.cpu().numpy()
        inside = np.zeros(len(host), bool)
        for o, n in self.off:
            inside[self.shift + o:self.shift + o + n] = True
        bad = np.flatnonzero(~inside & (host != GUARD_BYTE))
        assert len(bad) == 0, f"{len(bad)} guard bytes changed, the first at offset {int(bad[0]) - self.shift} of regions {self.off}"
        return [host[self.shift + o:self.shift + o + n].copy() for o, n in self.off]


def _unpack(order, tab, num, M, Lmax):
    return SimpleNamespace(num=int(num.view(np.int32)[0]), order=order.view(np.int64), table=tab.view(np.float64).reshape(Lmax, COLS),
                           table_words=tab.view(np.uint64).reshape(Lmax, COLS), order_words=order.view(np.uint64))


def on(stream):
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def table(points, labels, Lmax, stream=None):
    """one icpflow_cluster_table call -> num, order [M], table [Lmax, 9] (rows from num on still poison)"""
    M = len(labels)
    need = int(_lib._L.icpflow_cluster_table_workspace_bytes(M, Lmax))
    assert need > 0
    with on(stream):
        p, l = G(np.asarray(points, np.float32)), G(np.asarray(labels, np.float32))
        a = Arena([need, M * 8, Lmax * COLS * 8, 4])
        torch.cuda.current_stream().synchronize()
        t0 = time.perf_counter()
        rc = _lib._L.icpflow_cluster_table(_lib.ptr(p), _lib.ptr(l), M, a.ptr(1), a.ptr(2), Lmax, a.ptr(3), a.ptr(0), need, _lib.stream(DEV))
        assert rc == 0, (rc, _lib._L.icpflow_last_error())
        torch.cuda.current_stream().synchronize()
        seconds = time.perf_counter() - t0          # (enqueue and run of the chain, read by one test that prints it)
        _, order, tab, num = a.fetch()
    res = _unpack(order, tab, num, M, Lmax)
    res.seconds = seconds
    return res


def table_pair(pa, la, pb, lb, Lmax, stream=None):
    MA, MB = len(la), len(lb)
    need = int(_lib._L.icpflow_cluster_table_pair_workspace_bytes(MA, MB, Lmax))
    assert need > 0
    with on(stream):
        t = [G(np.asarray(x, np.float32)) for x in (pa, la, pb, lb)]
        a = Arena([need, MA * 8, Lmax * COLS * 8, 4, MB * 8, Lmax * COLS * 8, 4])
        rc = _lib._L.icpflow_cluster_table_pair(_lib.ptr(t[0]), _lib.ptr(t[1]), MA, a.ptr(1), a.ptr(2), a.ptr(3), _lib.ptr(t[2]), _lib.ptr(t[3]),
                                                MB, a.ptr(4), a.ptr(5), a.ptr(6), Lmax, a.ptr(0), need, _lib.stream(DEV))
        assert rc == 0, (rc, _lib._L.icpflow_last_error())
        torch.cuda.current_stream().synchronize()
        r = a.fetch()
    return _unpack(r[1], r[2], r[3], MA, Lmax), _unpack(r[4], r[5], r[6], MB, Lmax)


def cluster_stats(points, order, start, count, labels):
    """one icpflow_cluster_stats call (labels None: d_labels NULL) -> mean, extent float32 [L, 3]"""
    L = len(start)
    p, o = G(np.asarray(points, np.float32)), G(np.asarray(order, np.int64))
    s, c = G(np.asarray(start, np.int64)), G(np.asarray(count, np.int64))
    lab = G(np.asarray(labels, np.float32)) if labels is not None else None
    a = Arena([L * 12, L * 12])
    rc = _lib._L.icpflow_cluster_stats(_lib.ptr(p), _lib.ptr(o), _lib.ptr(s), _lib.ptr(c), _lib.ptr(lab), L, a.ptr(0), a.ptr(1), _lib.stream(DEV))
    assert rc == 0, (rc, _lib._L.icpflow_last_error())
    torch.cuda.synchronize()
    mean, ext = a.fetch()
    return mean.view(np.float32).reshape(L, 3), ext.view(np.float32).reshape(L, 3)

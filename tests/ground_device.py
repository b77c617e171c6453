"""What the GPU tests of icpflow_ground_segment share, in the style of tests/match_eval_device.py: the raw call through the C ABI
on buffers the test owns, with an icpflow_ground_params_t built from a ground_restatement.Params -- the points at any stride and
any 4-byte offset, the workspace of EXACTLY icpflow_ground_workspace_bytes(n, params) bytes, filled with 0xFF, between two guards,
the labels and the table between guards of their own, poisoned beforehand -- and compare(), the assertions of
tests/test_gpu_ground.py::compare at the case's own parameters.  Not a test module."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_restatement as gr      # noqa: E402
import residual_device as rd         # noqa: E402

GUARD, DEV = rd.GUARD, rd.DEV
WS_POISON, OUT_POISON = 0xFF, 0xA5
TABLE_BYTES = gr.PATCHES * gr.COLS * 8
TOL = 1e-9                           # tests/test_gpu_ground.py says why


def ground_params(params=None):
    """icpflow_ground_params_t of a ground_restatement.Params (the layout stays the library's own)"""
    from icp_flow_amd import _lib
    par, p = params or gr.DEFAULT, _lib.GroundParams.defaults()
    for name in ("sensor_height", "min_range", "max_range", "th_seeds", "th_dist", "th_seeds_v", "th_dist_v", "uprightness_thr",
                 "adaptive_seed_selection_margin", "num_iter", "num_lpr", "num_min_pts"):
        setattr(p, name, getattr(par, name))
    return p


def upload(pts, stride=3, offset=0, fill=np.nan):
    """-> (float32 tensor that holds the rows at `stride` floats from `offset` bytes on, every other word `fill`; the address of
    row 0)"""
    assert stride >= 3 and offset % 4 == 0
    n, lead = len(pts), offset // 4
    host = np.full(lead + n * stride + 1, fill, dtype=np.float32)
    host[lead: lead + n * stride].reshape(n, stride)[:, 0:3] = np.asarray(pts, dtype=np.float32)[:, 0:3]
    dev = torch.from_numpy(host).to(DEV)
    return dev, dev.data_ptr() + offset


class Buffers:
    """the workspace and the two outputs of one n, each between guards; poison() before a call, read() after it"""

    def __init__(self, n, params=None):
        from icp_flow_amd import _lib
        self.n, self.par = n, ground_params(params)
        self.need = int(_lib._L.icpflow_ground_workspace_bytes(n, ctypes.byref(self.par))) if n > 0 else 0
        assert n == 0 or self.need > 0
        self.sizes = dict(ws=self.need, labels=n, table=TABLE_BYTES)
        self.bufs = {k: rd._guarded(v, WS_POISON if k == "ws" else OUT_POISON) for k, v in self.sizes.items()}

    def poison_outputs(self):
        for k in ("labels", "table"):
            self.bufs[k][GUARD: GUARD + self.sizes[k]] = OUT_POISON

    def at(self, k):
        return ctypes.c_void_p(self.bufs[k].data_ptr() + GUARD)

    def inner(self, k):
        return self.bufs[k][GUARD: GUARD + self.sizes[k]].clone().cpu().numpy()


def run(pts, params=None, stride=3, offset=0, fill=np.nan, with_table=True, stream=None, buffers=None):
    """One call of icpflow_ground_segment -> (labels bool [n], table float64 [504, 16], or None without one).  Status 0, every
    guard intact, every label byte 0 or 1, every table word written.  `buffers`: those of an earlier call, the workspace as that
    call left it.  n == 0: status 0 and not a byte of any buffer changed."""
    from icp_flow_amd import _lib
    L, n = _lib._L, len(pts)
    b = buffers or Buffers(n, params)
    assert b.n == n
    b.poison_outputs()
    x, base = upload(pts, stride, offset, fill)
    before = {k: v.clone() for k, v in b.bufs.items()} if n == 0 or not with_table else None
    torch.cuda.synchronize()                                 # (the upload and the poison ran on the default stream)
    with torch.cuda.stream(stream):
        rc = L.icpflow_ground_segment(ctypes.c_void_p(base), stride, n, ctypes.byref(b.par), b.at("labels"), b.at("table") if with_table else None,
                                      b.at("ws"), ctypes.c_size_t(b.need), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    for k, buf in b.bufs.items():
        assert rd._guards_intact(buf, b.sizes[k]), f"guard of {k} changed"
    if n == 0:
        assert all(torch.equal(b.bufs[k], before[k]) for k in b.bufs), "n == 0 wrote something"
        return np.zeros(0, dtype=bool), None
    raw = b.inner("labels")
    assert ((raw == 0) | (raw == 1)).all(), f"{int(((raw != 0) & (raw != 1)).sum())} label bytes are neither 0 nor 1"
    if not with_table:
        assert torch.equal(b.bufs["table"], before["table"]), "a table that was not asked for was written"
        return raw.astype(bool), None
    words = b.inner("table").view(np.uint64)
    assert not (words == np.uint64(0xA5A5A5A5A5A5A5A5)).any(), "table words left unwritten"
    return raw.astype(bool), words.view(np.float64).reshape(gr.PATCHES, gr.COLS).copy()


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def compare(name, res, labels, table, params=None, leave_out=()):
    """tests/test_gpu_ground.py::compare at the case's parameters: the counts row for row, the labels on every row that is not in
    an undetermined patch, codes, ground counts, revert outcomes and removed points equal and the plane within TOL on every
    determined patch.  `leave_out`: patches that are named as degenerate, taken out of `determined` and of the labels.
    -> (rows compared, determined patches, the largest plane difference)"""
    par = params or gr.DEFAULT
    keep, det = gr.rows_to_compare(res, par), gr.determined(res, par)
    for p in leave_out:
        det[p] = False
        keep[res["patch"] == p] = False
    want = res["table"]
    diff = np.abs(table[det][:, 2:12] - want[det][:, 2:12])
    diff = diff[~(np.isnan(table[det][:, 2:12]) & np.isnan(want[det][:, 2:12]))]
    worst = float(diff.max()) if diff.size else 0.0
    wrong_counts = np.flatnonzero(table[:, 0] != want[:, 0])
    wrong_labels = np.flatnonzero(keep & (labels != res["nonground"]))
    print(f"{name}: rows {len(labels)}, compared {int(keep.sum())}, determined patches {int(det.sum())}, patches with another count "
          f"{len(wrong_counts)}, label mismatches {len(wrong_labels)}, max |plane - restatement| {worst:.3e}")
    assert not len(wrong_counts), (name, "counts", wrong_counts[:8], table[wrong_counts[:8], 0], want[wrong_counts[:8], 0])
    assert not len(wrong_labels), (name, "labels", wrong_labels[:8], res["patch"][wrong_labels[:8]])
    for col in (1, 12, 13, 14):
        bad = np.flatnonzero(det & (table[:, col] != want[:, col]))
        assert not len(bad), (name, "column", col, bad[:8], table[bad[:8], col], want[bad[:8], col])
    assert (np.isnan(table[det][:, 2:12]) == np.isnan(want[det][:, 2:12])).all(), name
    assert worst <= TOL, (name, worst)
    small = want[:, 0] < par.num_min_pts
    assert (table[small, 1:] == 0).all(), name
    return int(keep.sum()), int(det.sum()), worst

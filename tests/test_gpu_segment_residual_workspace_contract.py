"""The memory contract of icpflow_nn_residual_segments, in the style of tests/test_gpu_residual_workspace_contract.py: "the
caller owns the memory".  It runs on EXACTLY its *_workspace_bytes() bytes -- the documented formula, asserted here --, filled
with a poison, between two guards in the same allocation, each of its outputs between guards as well
(tests/segment_residual_device.py); asserted: status 0, every guard byte intact, the outputs bit-identical whatever the
workspace held and equal to the restatement, one byte too few refused with ICPFLOW_E_WORKSPACE with every output untouched, the
same result on a workspace that is 16- but not 256-byte aligned, one that is not 16-byte aligned (the records are float4)
refused, and the guards intact at every branch of the carve's use: d_d2_* given or NULL, E = 0 or 4, n or m = 0.

Who initialises what (csrc/segresid.hip): the call zeroes d_info and, per binning, the bucket counts (memsets on the stream);
the scan kernels write every tile word, every bucket's start and the number of rows in the table before the scatter and the
query read them; each side's scatter and query write every row of that side's d2 and of idx before its chunk kernel reads
them; the label order writes the order, the segments' rows and *d_num before the plan reads them, the plan writes chunkStart
before the chunk kernels do; every chunk's workgroup stores its whole partial of its side, and the final kernel reads only the
chunks the plan counts."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_residual_device as sd     # noqa: E402

pytestmark = pytest.mark.gpu
SIZES, M, LMAX = (2500, 1500, 700, 300), 3000, 64
N = sum(SIZES)
EDGES = (0.05, 0.1)


def _scene():
    return sd.scene(SIZES, M, seed=51, span=5.0, bad=True)


def test_the_size_is_the_documented_formula():
    from icp_flow_amd import _lib
    a = lambda x: -(-x // 256) * 256   # noqa: E731
    # a grid per cloud: 2^k >= twice its rows buckets (8192 for the 3000 targets, 16384 for the 5000 queries), 1024 buckets a
    # scan tile, one word for the rows in the table, 16 bytes a record -- ONE query grid for both sides; two d2 arrays and one idx
    # array; the order; 9 doubles a segment; the first chunk of every segment; 4 + 64 + 1 chunks of 2 x 8 doubles; the label
    # order's own workspace
    table = lambda H, rows: 2 * a(4 * H) + 4 * a(4 * (H // 1024)) + 256 + a(16 * rows)   # noqa: E731
    T = _lib._L.icpflow_cluster_table_workspace_bytes(N, LMAX)
    want = table(8192, M) + table(16384, N) + 3 * a(4 * N) + a(8 * N) + a(72 * LMAX) + a(4 * (LMAX + 1)) + a(128 * (N // 1024 + LMAX + 1)) + a(T)
    assert N == 5000 and T > 0
    assert _lib._L.icpflow_nn_residual_segments_workspace_bytes(N, M, LMAX, len(EDGES)) == want


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_runs_on_exactly_its_bytes_whatever_they_held(poison):
    b, a, f, lab, t = _scene()
    # one byte too few: refused before anything is written (sd.run compares every byte of every buffer)
    sd.run(b, a, f, lab, t, 1.0, EDGES, LMAX, ws_poison=poison, short=1, expect=-2, expect_message="icpflow_nn_residual_segments_workspace_bytes")
    got, _ = sd.check(b, a, f, lab, t, 1.0, EDGES, LMAX, ws_poison=poison, label=f"poison {poison:#x}")
    want = sd.run(b, a, f, lab, t, 1.0, EDGES, LMAX, ws_poison=0x3C)
    for k in ("table", "d2_before", "d2_after", "info"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["num"] == want["num"] == len(SIZES)


def test_workspace_at_base_plus_16():
    """a workspace that is 16- but not 256-byte aligned: every region is addressed relative to the base, the result is the same;
    base + 8 is refused with nothing written"""
    b, a, f, lab, t = _scene()
    want = sd.run(b, a, f, lab, t, 1.0, EDGES, LMAX)
    got = sd.run(b, a, f, lab, t, 1.0, EDGES, LMAX, shift=16)
    for k in ("table", "d2_before", "d2_after", "info"):
        assert got[k].tobytes() == want[k].tobytes(), k
    sd.run(b, a, f, lab, t, 1.0, EDGES, LMAX, shift=8, expect=-1, expect_message="16-byte aligned")


@pytest.mark.parametrize("outputs", [("d2_before", "d2_after"), ("d2_before",), ("d2_after",), ()], ids=["both", "before", "after", "neither"])
@pytest.mark.parametrize("edges", [(), (0.01, 0.05, 0.1, 1.0)], ids=["E0", "E4"])
def test_the_guards_stay_intact_at_the_carves_branches(outputs, edges):
    """(sd.run asserts every guard and that an output not asked for is untouched; sd.check the numbers)"""
    b, a, f, lab, t = _scene()
    sd.check(b, a, f, lab, t, 1.0, edges, LMAX, outputs=outputs, label=f"{outputs} {edges}")
    sd.check(b[:0], a[:0], f[:0], lab[:0], t, 1.0, edges, LMAX, outputs=outputs, label="n = 0")
    sd.check(b[:900], a[:900], f[:900], lab[:900], t[:0], 1.0, edges, LMAX, outputs=outputs, label="m = 0")
    sd.check(b[:0], a[:0], None, lab[:0], t[:0], 1.0, edges, 1, outputs=outputs, label="n = m = 0, Lmax = 1")

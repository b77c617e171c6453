"""The memory contract of icpflow_nn_residual, in the style of tests/test_gpu_buckets_workspace_contract.py: "the caller owns
the memory".  It runs on EXACTLY its *_workspace_bytes() bytes -- the documented formula, asserted here, not recorded numbers
--, filled with a poison, between two guards in the same allocation, each of its four outputs between guards as well
(tests/residual_device.py); asserted: status 0, every guard byte intact, the outputs bit-identical whatever the workspace held
and equal to the restatement, one byte too few refused with ICPFLOW_E_WORKSPACE before anything is written, the same result on
a workspace that is 16- but not 256-byte aligned, and a workspace that is not 16-byte aligned (the records are float4) refused.

Who initialises what (csrc/nnresid.hip): the call zeroes the bucket counts of both tables and d_info itself (memsets on the
stream), the scan kernels write every tile word, every bucket's start and the number of rows in the table before the scatter
and the query read them, the scatter writes exactly the records the query reads, the query writes every row of d2 and idx (in the workspace when the caller passes NULL)
before the table reads them, and every workgroup of the table stores its whole partial; nothing is read before it is written."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd             # noqa: E402

pytestmark = pytest.mark.gpu
N, M, G = 5000, 3000, 4
EDGES = (0.05, 0.1)


def _scene():
    return rd.scene(N, M, seed=51, span=5.0, radius=1.0, G=G, bad=True)


def test_the_size_is_the_documented_formula():
    from icp_flow_amd import _lib
    a = lambda x: -(-x // 256) * 256   # noqa: E731
    # a table per cloud: 2^k >= twice its rows buckets (8192 for the 3000 targets, 16384 for the 5000 queries), 1024 buckets a
    # scan tile, one word for the rows in the table, 16 bytes a record; a workgroup of the result table per 2048 query rows
    table = lambda H, rows: 2 * a(4 * H) + 4 * a(4 * (H // 1024)) + 256 + a(16 * rows)   # noqa: E731
    want = table(8192, M) + table(16384, N) + 2 * a(4 * N) + a(8 * 3 * G * (len(EDGES) + 4))
    assert _lib._L.icpflow_nn_residual_workspace_bytes(N, M, G, len(EDGES)) == want


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_runs_on_exactly_its_bytes_whatever_they_held(poison):
    q, t, f, g = _scene()
    # one byte too few: refused before anything is written
    rd.run(q, t, f, 1.0, g, G, EDGES, poison=poison, short=1, expect=-2, expect_message="icpflow_nn_residual_workspace_bytes")
    got, _ = rd.check(q, t, f, 1.0, g, G, EDGES, poison=poison, label=f"poison {poison:#x}")
    want = rd.run(q, t, f, 1.0, g, G, EDGES, poison=0x3C)
    for k in ("d2", "idx", "words", "info"):
        assert got[k].tobytes() == want[k].tobytes(), k
    # the rows the caller does not take live in the workspace: the table alone, on the same poison
    alone = rd.run(q, t, f, 1.0, g, G, EDGES, poison=poison, outputs=("table",))
    assert alone["words"].tobytes() == want["words"].tobytes() and alone["info"].tobytes() == want["info"].tobytes()


def test_workspace_at_base_plus_16():
    """a workspace that is 16- but not 256-byte aligned: every region is addressed relative to the base, the result is the same;
    base + 8 is refused with nothing written"""
    q, t, f, g = _scene()
    want = rd.run(q, t, f, 1.0, g, G, EDGES)
    got = rd.run(q, t, f, 1.0, g, G, EDGES, shift=16)
    for k in ("d2", "idx", "words", "info"):
        assert got[k].tobytes() == want[k].tobytes(), k
    rd.run(q, t, f, 1.0, g, G, EDGES, shift=8, expect=-1, expect_message="16-byte aligned")

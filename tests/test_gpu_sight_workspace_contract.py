"""The memory contract of icpflow_sight_segments (and of the two calls without a workspace beside it), in the style of
tests/test_gpu_segment_residual_workspace_contract.py: "the caller owns the memory".  The call runs on EXACTLY its
*_workspace_bytes() bytes -- the documented formula, asserted here --, filled with a poison, between two guards in the same
allocation, each of its outputs between guards as well (tests/sight_device.py); asserted: status 0, every guard byte intact, the
outputs bit-identical whatever the workspace held and equal to the restatement, one byte too few refused with
ICPFLOW_E_WORKSPACE with every output untouched, the same result on a workspace that is 16- but not 256-byte aligned, one that
is not 16-byte aligned refused, and the guards intact at every branch of the call: codes and distances given or NULL, n = 0.

Who initialises what (csrc/sight.hip): the call zeroes d_info (a memset on the stream); the label order writes the order, the
segments' rows and *d_num before the plan reads them, the plan writes chunkStart before the chunk kernel does; every chunk's
workgroup stores its whole partial, and the final kernel reads only the chunks the plan counts.  The build writes every word
of both planes of the image: the fill plane 0, the 3 x 3 pass plane 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sight_cases as cases              # noqa: E402
import sight_device as sd                # noqa: E402
import sight_restatement as S            # noqa: E402

pytestmark = pytest.mark.gpu
SIZES, M, LMAX = (2500, 1500, 700, 300), 3000, 64
N = sum(SIZES)
KEYS = ("table", "code_before", "code_after", "info")


def _scene():
    v = S.view(cases.ORIGIN)
    target = cases.sweep(M, 51, v, bad=True)
    before, flow, _ = cases.queries(N, 52, v, target, bad=True)
    rng = np.random.default_rng(53)
    labels = np.repeat(np.arange(len(SIZES), dtype=np.float32), SIZES)[rng.permutation(N)]
    d2 = [rng.choice(np.array([0.0, 0.005, 0.02, 4.0], np.float32), N) for _ in range(2)]
    image, _ = S.build(v, target)
    return image, before, flow, labels, d2[0], d2[1]


def test_the_size_is_the_documented_formula():
    from icp_flow_amd import _lib
    a = lambda x: -(-x // 256) * 256   # noqa: E731
    # the order; 9 doubles a segment; the first chunk of every segment; 4 + 64 + 1 chunks of 2 x 11 ints; the label order's own
    T = _lib._L.icpflow_cluster_table_workspace_bytes(N, LMAX)
    want = a(8 * N) + a(72 * LMAX) + a(4 * (LMAX + 1)) + a(88 * (N // 1024 + LMAX + 1)) + a(T)
    assert N == 5000 and T > 0
    assert _lib._L.icpflow_sight_segments_workspace_bytes(N, LMAX) == want


def _run(scene, **kw):
    image, before, flow, labels, d2b, d2a = scene
    return sd.segments(image, before, None, flow, labels, d2b, d2a, 0.1, LMAX, cases.ORIGIN, same_after=True, **kw)


@pytest.mark.parametrize("poison", [0x00, 0xA5, 0xFF], ids=["p00", "pA5", "pFF"])
def test_runs_on_exactly_its_bytes_whatever_they_held(poison):
    scene = _scene()
    image, before, flow, labels, d2b, d2a = scene
    # one byte too few: refused before anything is written (sd.segments compares every byte of every buffer)
    _run(scene, ws_poison=poison, short=1, expect=-2, expect_message="icpflow_sight_segments_workspace_bytes")
    got = _run(scene, ws_poison=poison)
    sd.compare_segments(got, S.segments(S.view(cases.ORIGIN), image, before, before, flow, labels, d2b, d2a, 0.1), f"poison {poison:#x}")
    want = _run(scene, ws_poison=0x3C)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["num"] == want["num"] == len(SIZES)


def test_workspace_at_base_plus_16():
    """a workspace that is 16- but not 256-byte aligned: every region is addressed relative to the base, the result is the same;
    base + 8 is refused with nothing written"""
    scene = _scene()
    want, got = _run(scene), _run(scene, shift=16)
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    _run(scene, shift=8, expect=-1, expect_message="16-byte aligned")


@pytest.mark.parametrize("outputs", [("code_before", "code_after"), ("code_before",), ("code_after",), ()], ids=["both", "before", "after", "neither"])
@pytest.mark.parametrize("distances", [True, False], ids=["d2", "no-d2"])
def test_the_guards_stay_intact_at_the_calls_branches(outputs, distances):
    """(sd.segments asserts every guard and that an output not asked for is untouched; compare_segments the numbers)"""
    image, before, flow, labels, d2b, d2a = _scene()
    v = S.view(cases.ORIGIN)
    d2 = (d2b, d2a) if distances else (None, None)
    for rows, Lmax, label in ((N, LMAX, "all rows"), (0, LMAX, "n = 0"), (900, 4, "900 rows, Lmax = 4"), (0, 1, "n = 0, Lmax = 1")):
        cut = lambda x: None if x is None else x[:rows]    # noqa: E731
        got = sd.segments(image, cut(before), None, cut(flow), cut(labels), cut(d2[0]), cut(d2[1]), 0.1, Lmax, cases.ORIGIN, outputs=outputs, same_after=True)
        sd.compare_segments(got, S.segments(v, image, cut(before), cut(before), cut(flow), cut(labels), cut(d2[0]), cut(d2[1]), 0.1), label)


def test_the_build_writes_every_word_of_the_image_and_the_query_only_its_rows():
    """whatever the image's memory held; the refusals of the calls without a workspace leave every byte as it was"""
    v = S.view(cases.ORIGIN, W=8, H=3)
    target = cases.sweep(300, 55, v, bad=True)
    want, info = S.build(v, target)
    for poison in (0x00, 0xA5, 0xFF):
        got = sd.build(target, cases.ORIGIN, poison=poison, W=8, H=3)
        assert np.array_equal(got["image"], want) and tuple(got["info"].tolist()) == info
    sd.build(target, cases.ORIGIN, expect=-1, expect_message="W = 6", W=6, H=3)
    sd.build(target, (0, 0, float("nan")), expect=-1, expect_message="h_origin[2]", W=8, H=3)
    q, f, _ = cases.queries(257, 56, v, target, bad=True)
    sd.query(want, q, f, cases.ORIGIN, expect=-1, expect_message="margin_rel", W=8, H=3, margin_rel=1.0)

"""CPU-only: the line-of-sight check (icpflow_sight_build / _query / _segments, csrc/sight.hip; utils_eval.sight_image,
line_of_sight, segment_sight; run_stream's `--residual-sight`) as far as it goes without a GPU -- the exports, every refusal
with its code and message (all of them come before any launch), the pinned size query against the header's formula, the
command line, SegmentSight.annotate on a hand-made table, the restatement the GPU tests compare against
(tests/sight_restatement.py) against the same map in exact rationals and on a scene counted by hand, and the conditions the GPU
tests' scenes must meet (tests/sight_cases.py), asserted on the restatement."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_residual_restatement as sr     # noqa: E402
import sight_cases as cases                   # noqa: E402
import sight_restatement as S                 # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "workspace_sizes_sight.json")
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
F = np.float32
NAMES = ("icpflow_sight_default_params", "icpflow_sight_build", "icpflow_sight_query", "icpflow_sight_segments_workspace_bytes",
         "icpflow_sight_segments")


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib, build
    assert _lib.VERSION == 215
    for name, n_args in zip(NAMES, (1, 7, 10, 2, 20)):
        assert hasattr(_lib._L, name) and len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES["icpflow_sight_segments_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.SIGHT_COLS, _lib.SIGHT_MAX_SEGMENTS, ctypes.sizeof(_lib.SightParams)) == (24, 4096, 64)
    assert "sight.hip" in build.SOURCES and "sight.hpp" in build.HEADERS
    hdr = open(os.path.join(REPO, "include", "icpflow_hip.h")).read()
    assert "#define ICPFLOW_SIGHT_COLS 24" in hdr and all(name + "(" in hdr for name in NAMES)
    for k, name in enumerate(("OUTSIDE", "NO_RETURN", "SEEN_THROUGH", "AT_FIRST_RETURN", "BEHIND")):
        assert f"#define ICPFLOW_SIGHT_{name} {k}" in hdr and getattr(_lib, "SIGHT_" + name) == k
    p = _lib.SightParams.defaults()
    assert p.struct_size == 64 and p.as_dict() == S.START
    assert (S.OUTSIDE, S.NO_RETURN, S.SEEN_THROUGH, S.AT_FIRST_RETURN, S.BEHIND, S.BAD) == (0, 1, 2, 3, 4, _lib.SIGHT_BAD_ROW)
    with pytest.raises(TypeError, match="no parameter"):
        _lib.SightParams.defaults(width=3)


ONE = ctypes.c_void_p(4096)


def _origin(o):
    return np.ascontiguousarray(o, dtype=np.float64)


def _build(**over):
    from icp_flow_amd import _lib
    a = dict(target=ONE, m=10, origin=(0, 0, 0), image=ONE, info=ONE, params={})
    a.update(over)
    p = a["params"] if a["params"] is None or isinstance(a["params"], _lib.SightParams) else _lib.SightParams.defaults(**a["params"])
    o = None if a["origin"] is None else _origin(a["origin"])
    rc = _lib._L.icpflow_sight_build(a["target"], a["m"], None if o is None else o.ctypes.data_as(ctypes.c_void_p), None if p is None else ctypes.byref(p),
                                     a["image"], a["info"], None)
    return rc, _lib._L.icpflow_last_error().decode()


def _query(**over):
    from icp_flow_amd import _lib
    a = dict(image=ONE, params={}, origin=(0, 0, 0), query=ONE, flow=None, n=10, code=ONE, near=None, counts=ONE)
    a.update(over)
    p = a["params"] if a["params"] is None or isinstance(a["params"], _lib.SightParams) else _lib.SightParams.defaults(**a["params"])
    o = None if a["origin"] is None else _origin(a["origin"])
    rc = _lib._L.icpflow_sight_query(a["image"], None if p is None else ctypes.byref(p), None if o is None else o.ctypes.data_as(ctypes.c_void_p),
                                     a["query"], a["flow"], a["n"], a["code"], a["near"], a["counts"], None)
    return rc, _lib._L.icpflow_last_error().decode()


def _segments(**over):
    """the call with arguments that pass every check but the workspace's size (16 bytes: nothing is launched)"""
    from icp_flow_amd import _lib
    a = dict(image=ONE, params={}, origin=(0, 0, 0), before=ONE, after=ONE, flow=None, labels=ONE, n=10, d2b=ONE, d2a=ONE, far=0.1, table=ONE,
             Lmax=64, num=ONE, cb=None, ca=None, info=ONE, ws=ONE, ws_bytes=16)
    a.update(over)
    p = a["params"] if a["params"] is None or isinstance(a["params"], _lib.SightParams) else _lib.SightParams.defaults(**a["params"])
    o = None if a["origin"] is None else _origin(a["origin"])
    rc = _lib._L.icpflow_sight_segments(a["image"], None if p is None else ctypes.byref(p), None if o is None else o.ctypes.data_as(ctypes.c_void_p),
                                        a["before"], a["after"], a["flow"], a["labels"], a["n"], a["d2b"], a["d2a"], a["far"], a["table"], a["Lmax"],
                                        a["num"], a["cb"], a["ca"], a["info"], a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    return rc, _lib._L.icpflow_last_error().decode()


BAD_PARAMS = (("W", dict(W=0)), ("W", dict(W=6)), ("W", dict(W=8196)), ("W", dict(W=-4)), ("H", dict(H=0)), ("H", dict(H=2049)),
              ("2^22", dict(W=8192, H=1024)), ("tan_lo", dict(tan_lo=0.4)), ("tan_lo", dict(tan_lo=0.5)), ("tan_lo", dict(tan_lo=float("nan"))),
              ("tan_hi", dict(tan_hi=float("inf"))), ("tan_lo", dict(tan_lo=0.4 - 1e-12)), ("min_range", dict(min_range=-1.0)),
              ("min_range", dict(min_range=200.0)), ("max_range", dict(max_range=1.5e6)), ("max_range", dict(max_range=float("nan"))),
              ("margin_abs", dict(margin_abs=-0.1)), ("margin_abs", dict(margin_abs=float("inf"))), ("margin_rel", dict(margin_rel=1.0)),
              ("margin_rel", dict(margin_rel=-0.01)), ("margin_rel", dict(margin_rel=float("nan"))))


def test_every_refusal_has_its_code_and_message():
    from icp_flow_amd import _lib
    # what passes every argument check of the segments' call stops at the workspace: the refusals below are not that one
    rc, msg = _segments()
    assert rc == E_WORKSPACE and "icpflow_sight_segments_workspace_bytes" in msg
    rc, msg = _segments(ws=None, ws_bytes=1 << 30)
    assert rc == E_WORKSPACE and "workspace" in msg
    for call, fn, required in ((_build, "icpflow_sight_build", ("target", "origin", "image", "info", "params")),
                               (_query, "icpflow_sight_query", ("image", "params", "origin", "query", "code", "counts")),
                               (_segments, "icpflow_sight_segments", ("image", "params", "origin", "before", "after", "labels", "table", "num", "info"))):
        for name in required:
            rc, msg = call(**{name: None})
            assert rc == E_ARG and fn + ": null pointer" in msg, (fn, name)
        size = "m" if call is _build else "n"
        rc, msg = call(**{size: -1})
        assert rc == E_ARG and f"{size} < 0" in msg and fn in msg
        rc, msg = call(**{size: (1 << 29) + 1})
        assert rc == E_LIMIT and "rows a cloud" in msg and fn in msg
        for word, over in BAD_PARAMS:
            rc, msg = call(params=over)
            assert rc == E_ARG and word in msg and fn in msg, (fn, over, msg)
        p = _lib.SightParams.defaults()
        p.struct_size = 56
        rc, msg = call(params=p)
        assert rc == E_ARG and "struct_size = 56" in msg and fn in msg
        for o in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, 1.5e6)):
            rc, msg = call(origin=o)
            assert rc == E_ARG and "h_origin" in msg and fn in msg, o
    # a cloud without rows needs no pointer; the optional arguments may be NULL, each and together
    assert _segments(before=None, after=None, labels=None, n=0)[0] == E_WORKSPACE
    for over in (dict(d2b=None), dict(d2a=None), dict(d2b=None, d2a=None), dict(flow=ONE), dict(cb=ONE), dict(ca=ONE), dict(cb=ONE, ca=ONE),
                 dict(origin=(0.5, -3, 1.7)), dict(params=dict(W=4, H=1)), dict(params=dict(W=8192, H=512)), dict(params=dict(W=2048, H=2048)),
                 dict(params=dict(min_range=0.0, max_range=1e6, margin_abs=0.0, margin_rel=0.0)), dict(far=0.0), dict(far=1e3)):
        assert _segments(**over)[0] == E_WORKSPACE, over
    for far in (-0.1, 1000.5, float("nan"), float("inf")):
        rc, msg = _segments(far=far)
        assert rc == E_ARG and "far must lie in [0, 1e3]" in msg, far
    for Lmax in (0, -1):
        rc, msg = _segments(Lmax=Lmax)
        assert rc == E_ARG and "Lmax must be at least 1" in msg, Lmax
    for Lmax in (4097, 1 << 20):
        rc, msg = _segments(Lmax=Lmax)
        assert rc == E_LIMIT and "at most 4096 segments" in msg, Lmax
    assert _segments(Lmax=1)[0] == E_WORKSPACE and _segments(Lmax=4096)[0] == E_WORKSPACE
    need = _lib._L.icpflow_sight_segments_workspace_bytes(10, 64)
    rc, msg = _segments(ws=ctypes.c_void_p(4096 + 8), ws_bytes=need)
    assert rc == E_ARG and "16-byte aligned" in msg
    assert _lib._L.icpflow_sight_default_params(None) == E_ARG and "null pointer" in _lib._L.icpflow_last_error().decode()


def _formula(n, Lmax):
    """the size as include/icpflow_hip.h states it"""
    from icp_flow_amd import _lib
    a = lambda x: -(-x // 256) * 256   # noqa: E731
    chunks = n // 1024 + min(n, Lmax) + 1
    T = _lib._L.icpflow_cluster_table_workspace_bytes(max(n, 1), Lmax)
    return a(8 * n) + a(72 * Lmax) + a(4 * (Lmax + 1)) + a(88 * chunks) + a(T)


def test_the_size_query_is_pinned_and_monotone():
    from icp_flow_amd import _lib
    q = _lib._L.icpflow_sight_segments_workspace_bytes
    recorded = json.load(open(GOLDEN))["icpflow_sight_segments_workspace_bytes"]
    assert len(recorded) >= 100
    for n, Lmax, size in recorded:
        assert q(n, Lmax) == size == _formula(n, Lmax) and size % 256 == 0 and size > 0, (n, Lmax)
    sizes = [0, 1, 63, 64, 65, 511, 512, 513, 2049, 20000, 63276, 130000, 1 << 20]
    for Lmax in (1, 64, 4096):
        by_n = [q(n, Lmax) for n in sizes]
        assert by_n == sorted(by_n), Lmax
    for n in sizes:
        by_l = [q(n, Lmax) for Lmax in (1, 2, 64, 65, 1000, 4096)]
        assert by_l == sorted(by_l), n
    assert q(-1, 1) == 0 and q(1, 0) == 0 and q(1, 4097) == 0 and q((1 << 29) + 1, 1) == 0


def test_there_is_no_cpu_path():
    from icp_flow_amd import _lib, utils_eval
    x, lab = torch.zeros(8, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.sight_image(x)
    image = utils_eval.SightImage(torch.zeros((2, 64, 1024), dtype=torch.int32), _lib.SightParams.defaults(), (0, 0, 0), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.line_of_sight(image, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.segment_sight_device(image, x, x, None, lab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.segment_sight(image, x, x, x, lab)


def test_the_flag_parses_bare_and_with_an_origin():
    from icp_flow_amd import frame_pairs
    ap = frame_pairs.argument_parser()
    assert ap.parse_args(["dir"]).residual_sight is None
    assert ap.parse_args(["dir", "--residual", "--residual-segments", "--residual-sight"]).residual_sight == []
    ns = ap.parse_args(["dir", "--residual", "0.5", "--residual-segments", "worst.json", "--residual-sight", "0", "-0.5", "1.7"])
    assert ns.residual_sight == [0.0, -0.5, 1.7] and ns.residual_segments == "worst.json" and ns.residual == 0.5
    for argv in (["dir", "--residual-sight"], ["dir", "--residual", "--residual-sight"], ["dir", "--residual-sight", "0", "0", "1.5"]):
        with pytest.raises(SystemExit, match="--residual-sight goes with --residual-segments"):
            frame_pairs.main(argv)
    with pytest.raises(SystemExit, match="the origin's three"):
        frame_pairs.main(["dir", "--residual", "--residual-segments", "--residual-sight", "1", "2"])
    assert "residual_sight" not in frame_pairs.DEFAULT_ARGS and not hasattr(frame_pairs.default_args(), "residual_sight")


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _dyadic_points(count, seed, origin):
    """points whose coordinates are multiples of 2^-6 within +-64 m: exact as floats and as rationals"""
    rng = np.random.default_rng(seed)
    p = rng.integers(-4096, 4097, (count, 3)).astype(np.float64) / 64.0
    p[:, 2] = rng.integers(-1024, 1025, count) / 64.0
    return (p + np.asarray(origin, np.float64)).astype(F)


@pytest.mark.parametrize("shape,origin", [((1024, 64), (0, 0, 0)), ((8, 3), (0, 0, 0)), ((2048, 128), cases.ORIGIN), ((4, 1), cases.ORIGIN)])
def test_the_float32_map_agrees_with_exact_rationals_clear_of_borders(shape, origin):
    """Where a point lies at least 1e-3 of a pixel from every border of its pixel, the float32 map -- a dozen operations of
    relative error 2^-24 each -- cannot land in another pixel than the exact one (1e-3 of a pixel of a 2048 x 128 image is a
    relative 1e-3 / 2048 = 5e-7 of p's range, 8 times 2^-24); on borders the rounding decides, and the next test pins it."""
    v = S.view(origin, W=shape[0], H=shape[1])
    pts = _dyadic_points(6000 if shape[0] > 8 else 600, 7 + shape[0], origin)
    row, col, _, _, _ = S.pixel(v, pts)
    checked = 0
    for k, p in enumerate(pts):
        e = S.exact_pixel(v, p)
        if e is None:
            if (np.abs(p[:2].astype(np.float64) - np.asarray(origin[:2])) > 0).any():   # off the axis: outside by the elevation
                t = (float(p[2]) - origin[2]) / np.hypot(float(p[0]) - origin[0], float(p[1]) - origin[1])
                if abs(t - float(v["tan_lo"])) > 1e-5 and abs(t - float(v["tan_hi"])) > 1e-5:
                    assert row[k] == -1, (k, p)
                    checked += 1
            continue
        if e[2] < 1e-3:
            continue
        rho = np.linalg.norm(p.astype(np.float64) - np.asarray(origin))
        if rho < float(v["min_range"]) * 1.001 or rho > float(v["max_range"]) * 0.999:
            continue
        assert (row[k], col[k]) == (e[0], e[1]), (k, p, e, row[k], col[k])
        checked += 1
    assert checked >= (5000 if shape[0] > 8 else 400), checked


@pytest.mark.parametrize("origin", [(0, 0, 0), cases.ORIGIN])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_on_the_borders_the_decision_is_the_one_the_header_states(shape, origin):
    W, H = shape
    v = S.view(origin, W=W, H=H)
    named = cases.border_points(v)
    pts = np.stack([p for _, p in named])
    row, col, rho, p, t = S.pixel(v, pts)
    at = {name: k for k, (name, _) in enumerate(named)}
    mid_row = row[at["column 0"]]
    assert mid_row >= 0
    assert (row[at["column 0"]], col[at["column 0"]]) == (mid_row, 0) and col[at["column W - 1"]] == W - 1
    assert p[at["p rounds to 4"]] == F(4) and col[at["p rounds to 4"]] == 0                   # col == W wraps to 0
    assert col[at["quadrant 2"]] == W // 2 - 1 and col[at["quadrant 3"]] == W // 2             # p = 2 - g on either side of 2
    assert p[at["ux = -0"]] == F(1) and col[at["ux = -0"]] == W // 4                           # -0.0 counts as >= 0
    assert col[at["uy = -0"]] == 0 and row[at["uy = -0"]] == mid_row
    assert t[at["t == tan_lo"]] == v["tan_lo"] and row[at["t == tan_lo"]] == 0 and row[at["row 0"]] == 0
    assert row[at["below tan_lo"]] == -1 and t[at["below tan_lo"]] < v["tan_lo"]
    assert t[at["row H - 1"]] == np.nextafter(v["tan_hi"], F(-np.inf)) and row[at["row H - 1"]] == H - 1 and col[at["row H - 1"]] == W // 4
    assert t[at["t == tan_hi"]] == v["tan_hi"] and row[at["t == tan_hi"]] == -1                # the upper bound is exclusive
    assert row[at["vertical axis"]] == -1 and row[at["vertical axis, -0"]] == -1
    assert (row[at["far corner"]], col[at["far corner"]]) == (H - 1, W // 2)
    for name, r in (("min_range", v["min_range"]), ("max_range", v["max_range"])):
        ks = [at[f"rho {name} {k:+d}"] for k in (-2, -1, 0, 1, 2)]
        assert rho[ks[2]] == r and row[ks[2]] >= 0                                             # rho == the bound is inside
        assert rho[ks[0]] < r < rho[ks[4]]
        outside = [row[k] == -1 for k in ks]
        assert outside == [bool(rho[k] < r) if name == "min_range" else bool(rho[k] > r) for k in ks] and any(outside)
    # the image of these points: the columns wrap and the rows clip in the 3 x 3 plane
    image, info = S.build(v, pts)
    assert info[0] == 0 and info[1] == int((row == -1).sum()) and info[2] == len({(r, c) for r, c in zip(row, col) if r >= 0})
    plane0, plane1 = image[0].view(F), image[1].view(F)
    k = at["column W - 1"]
    assert plane0[mid_row, W - 1] == rho[k] and plane1[mid_row, 0] <= rho[k] and plane1[mid_row, W - 2] <= rho[k]
    assert plane1[mid_row, W - 1] <= min(rho[k], plane0[mid_row, 0])                           # column W - 1 sees column 0
    assert plane1[0, W // 2] == plane0[:2, [W // 2 - 1, W // 2, (W // 2 + 1) % W]].min()       # row -1 does not exist
    assert plane1[H - 1, W // 4] == plane0[max(H - 2, 0):, [W // 4 - 1, W // 4, W // 4 + 1]].min()
    assert (plane1 <= plane0).all() and np.isinf(plane0).any() == (info[2] < W * H)


def test_a_scene_of_three_segments_counted_by_hand():
    """W = 8, H = 2, tan in [-1, 1): rows split at t = 0; columns are the eight half-quadrants.  Margins 0.5 m + 0: thr = 0.5.
    Targets: (8, 1, 1) -> col 0, row 1, rho = sqrt(66); (8, 1, -1) -> col 0, row 0; (-4, 0, 1) -> col 4 (p = 2), row 1, rho =
    sqrt(17); a pad row."""
    v = S.view((0, 0, 0), W=8, H=2, tan_lo=-1.0, tan_hi=1.0, min_range=1.0, max_range=100.0, margin_abs=0.5, margin_rel=0.0)
    target = np.array([[8, 1, 1], [8, 1, -1], [-4, 0, 1], [1e8, 1e8, 1e8]], F)
    image, info = S.build(v, target)
    assert info == (1, 0, 3)
    r66, r17 = np.sqrt(F(66)), np.sqrt(F(17))
    plane0 = image[0].view(F)
    assert plane0[1, 0] == r66 and plane0[0, 0] == r66 and plane0[1, 4] == r17 and np.isinf(plane0).sum() == 13
    plane1 = image[1].view(F)
    assert (plane1[:, [7, 0, 1]] == r66).all() and (plane1[:, [3, 4, 5]] == r17).all() and np.isinf(plane1[:, [2, 6]]).all()
    before = np.array([[4, 0.5, 0.5],      # label 5: col 0, rho = sqrt(16.5) = 4.06 + 0.5 < 8.12: seen through
                       [8, 1, 1],          # label 5: on the return: at the first return
                       [16, 2, 2],         # label 5: rho = 2 sqrt(66): behind
                       [0, 4, 1],          # label -1: col 2: no return
                       [0, 0, 3],          # label -1: on the axis: outside
                       [0.5, 0, 0],        # label -1: rho 0.5 < min_range: outside
                       [np.nan, 0, 0],     # label 7: bad on both sides
                       [-2, 0, 0.5]],      # label 7: col 4, rho = sqrt(4.25) = 2.06 + 0.5 < 4.12: seen through; the flow takes it to
                      F)                   #          (-4, 0, 1): at the first return
    flow = np.zeros((8, 3), F)
    flow[7] = (-2, 0, 0.5)
    flow[3] = (np.inf, 0, 0)               # bad AFTER only
    labels = np.array([5, 5, 5, -1, -1, -1, 7, 7], F)
    d2 = np.array([4.0, 0.0, 4.0, 4.0, 0.005, 4.0, 4.0, 0.02], F)          # far = 0.1: d2 > 0.01
    res = S.segments(v, image, before, before, flow, labels, d2, d2, far=0.1)
    assert res["code_before"].tolist() == [2, 3, 4, 1, 0, 0, -2, 2] and res["code_after"].tolist() == [2, 3, 4, -2, 0, 0, -2, 3]
    assert res["labels"].tolist() == [-1.0, 5.0, 7.0] and res["rows"].tolist() == [3, 3, 2]
    assert res["info"] == [1, 2, 1, 2, 1, 1, 2, 2, 0, 1, 2, 1]
    t = res["table"]
    assert t.shape == (3, 24)
    #                      label rows good  0     1     2     3     4   | good  0     1     2     3     4
    assert t[0].tolist() == [-1, 3, 3, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 2, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert t[1].tolist() == [5, 3, 3, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1, 3, 0, 0, 0, 0, 1, 1, 1, 0, 1, 1]
    assert t[2].tolist() == [7, 2, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    # without the distances no row is far; the query's codes and counts are the segments'
    bare = S.segments(v, image, before, before, flow, labels)["table"]
    assert (bare[:, 4:13:2] == 0).all() and (bare[:, 15:24:2] == 0).all() and np.array_equal(bare[:, 3:13:2], t[:, 3:13:2])
    code, near, counts = S.query(v, image, before, flow)
    assert code.tolist() == res["code_after"].tolist() and counts == res["info"][6:]
    assert near[0] == r66 and near[7] == r17 and np.isinf(near[[3, 4, 5, 6]]).all()
    # the host-side class reads that table
    from icp_flow_amd import utils_eval
    s = utils_eval.SegmentSight.from_table(t, dict(after_seen_through=1))
    assert s.labels.tolist() == [-1, 5, 7] and s.rows.tolist() == [3, 3, 2] and len(s) == 3
    assert s.before.good.tolist() == [3, 3, 1] and s.after.codes[1].tolist() == [0, 0, 1, 1, 1] and s.after.far[1].tolist() == [0, 0, 1, 0, 1]
    assert s.far_rows(1) == 2 and s.seen_through_share(1) == 0.5 and s.excused_share(1) == 0.5 and s.far_rows(0) == 1 and s.excused_share(0) == 1.0


def _hand_sight():
    """six segments, AFTER side's FAR rows per code (outside, no return, seen through, at first return, behind)"""
    far = {0.0: (0, 0, 6, 2, 2), 1.0: (2, 2, 1, 1, 3), 2.0: (0, 0, 5, 0, 5), 3.0: (0, 0, 0, 0, 0), 4.0: (1, 0, 1, 8, 0), 5.0: (0, 5, 4, 1, 0)}
    t = np.zeros((len(far), 24))
    for k, (label, row) in enumerate(far.items()):
        t[k, 0], t[k, 1], t[k, 13] = label, 20, 20
        t[k, 14:24:2] = np.asarray(row) + 2           # the rows of the code: the far ones and two more
        t[k, 15:24:2] = row
    return t


def test_annotate_takes_majorities_and_leaves_ties_undecided():
    from icp_flow_amd import utils_eval
    s = utils_eval.SegmentSight.from_table(_hand_sight())
    entries = [dict(label=float(k), rows=20, after_mean=0.5, before_mean=0.6, gain=0.1, hit_rate_after=0.5, matched=False, pair=None) for k in range(6)]
    keys = list(entries[0])
    out = s.annotate(entries)
    assert out is entries and list(entries[0]) == keys + ["seen_through", "excused", "far_rows", "verdict"]
    assert [e["verdict"] for e in entries] == ["seen through", "lost from view", "undecided", "undecided", "undecided", "undecided"]
    assert [e["far_rows"] for e in entries] == [10, 9, 10, 0, 10, 10] and [e["seen_through"] for e in entries] == [6, 1, 5, 0, 1, 4]
    assert [e["excused"] for e in entries] == [2, 7, 5, 0, 1, 5]              # 2: a 50 / 50 tie; 3: no far row; 4: most at the first return
    assert [e["verdict"] for e in s.annotate([dict(label=5.0), dict(label=0.0)], share=0.4)] == ["lost from view", "seen through"]
    assert [e["verdict"] for e in s.annotate([dict(label=0.0)], share=0.6)] == ["undecided"]
    with pytest.raises(ValueError, match="no segment with label"):
        s.annotate([dict(label=9.0)])
    lines = utils_eval.format_segment_sight(entries)
    assert len(lines) == 6 and lines[0].startswith("residual segment:   0, after: 0.5000") and lines[0].endswith("far rows:     10, seen through:      6, excused:      2, seen through")
    assert utils_eval.SIGHT_VERDICTS == ("seen through", "lost from view", "undecided")


def _stub_register(args, fp, device):
    return dict(pairs=torch.zeros((2, 10)), transformations=torch.eye(4).repeat(2, 1, 1), flow=torch.from_numpy(fp.gt_flow.copy()))


def test_without_the_attribute_the_summary_has_todays_keys():
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=1, n_objects=3, n_max=60, n_background=50)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    a = frame_pairs.default_args()
    s = frame_pairs.run_stream(a, [fp, fp], "cpu", register_fn=_stub_register)
    assert list(s) == ["frame_pairs", "matched_cluster_pairs", "n_gpus", "ms_per_frame_pair", "frame_pairs_per_s", "evaluated_points",
                       "pose_sources", "epe", "accs", "accr", "outlier", "Routlier"]
    a.residual_sight = None                      # as good as absent
    assert list(frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)) == list(s)
    for value in (True, (0.0, 0.0, 1.5)):
        a.residual_sight = value
        with pytest.raises(ValueError, match="needs args.residual_segments"):
            frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    a.residual, a.residual_segments = 2.0, True
    a.residual_sight = (0.0, 1.0)
    with pytest.raises(ValueError, match="an origin"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    a.residual_sight = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    assert callable(frame_pairs.frame_segment_sight)


NEEDS_RESIDUAL = "args.residual_segments needs args.residual: the two share the radius"
SEGMENTS_ONE_RANK = "args.residual_segments under more than one rank: merging the lists is not built"
NEEDS_SEGMENTS = "args.residual_sight needs args.residual_segments: it judges the segments that one lists"
AN_ORIGIN = "args.residual_sight: True or an origin (x, y, z), got (0.0, 1.0)"
TRUST_NEEDS = "args.residual_trust needs args.residual and args.residual_segments: it spreads their verdicts over the rows"
OBJECTS_ONE_RANK = "args.objects under more than one rank: merging the files is not built"
TRACKS_ONE_RANK = "args.tracks under more than one rank: a sample's gaps would have to meet on one rank, which is not built"
WITH_SEGMENTS = dict(residual=2.0, residual_segments=True)
# (attributes, world, the message): run_stream checks in the order residual_segments (its residual, then the ranks), residual_sight
# (its segments, then the origin), residual_trust, objects, tracks -- read off the run_stream that held all of this in one function --
# and the first complaint wins
WRONG = [
    (dict(residual_segments=True), 1, NEEDS_RESIDUAL),
    (dict(residual_sight=True), 1, NEEDS_SEGMENTS),
    (dict(residual=2.0, residual_sight=(0.0, 0.0, 1.5)), 1, NEEDS_SEGMENTS),
    (dict(residual_trust=True), 1, TRUST_NEEDS),
    (dict(residual=2.0, residual_trust=True), 1, TRUST_NEEDS),
    (dict(WITH_SEGMENTS, residual_sight=(0.0, 1.0)), 1, AN_ORIGIN),
    (WITH_SEGMENTS, 2, SEGMENTS_ONE_RANK),
    (dict(objects=True), 2, OBJECTS_ONE_RANK),
    (dict(tracks="tracks.jsonl"), 2, TRACKS_ONE_RANK),
    # two at once
    (dict(residual_segments=True), 2, NEEDS_RESIDUAL),
    (dict(residual_segments="worst.json", residual_sight=(0.0, 1.0), residual_trust=True, objects=True), 2, NEEDS_RESIDUAL),
    (dict(residual_sight=(0.0, 1.0)), 1, NEEDS_SEGMENTS),
    (dict(residual_sight=True, residual_trust=True), 1, NEEDS_SEGMENTS),
    (dict(WITH_SEGMENTS, residual_sight=(0.0, 1.0)), 2, SEGMENTS_ONE_RANK),
    (dict(WITH_SEGMENTS, objects=True, tracks=True), 2, SEGMENTS_ONE_RANK),
    (dict(residual_sight=(0.0, 1.0), objects=True), 2, NEEDS_SEGMENTS),
    (dict(residual_trust=True, objects=True, tracks=True), 2, TRUST_NEEDS),
    (dict(objects=True, tracks=True), 2, OBJECTS_ONE_RANK),
]


@pytest.mark.parametrize("attributes, world, message", WRONG)
def test_every_wrong_combination_keeps_its_message_and_its_turn(attributes, world, message):
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=1, n_objects=3, n_max=60, n_background=50)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    a = frame_pairs.default_args()
    for name, value in attributes.items():
        setattr(a, name, value)
    with pytest.raises(ValueError) as refusal:          # (before any frame pair is registered, and before any collective)
        frame_pairs.run_stream(a, [fp, fp], "cpu", world=world, register_fn=_stub_register)
    assert str(refusal.value) == message


# ---- the conditions of the GPU tests' scenes ----------------------------------------------------------------------------------
def test_the_sweeps_cover_every_code_and_the_bad_rows():
    v = S.view(cases.ORIGIN)
    target = cases.sweep(2049, 11, v, bad=True)
    image, info = S.build(v, target)
    assert info[0] >= 6 and info[1] > 50 and info[2] > 1000
    q, f, spoiled = cases.queries(2049, 12, v, target, bad=True)
    code, near, counts = S.query(v, image, q, f)
    assert all(c > 20 for c in counts[1:]) and counts[0] >= 8 + len(spoiled) and sum(counts) == 2049
    assert len(spoiled) >= 4 and S.good(q[spoiled]).all() and (code[spoiled] == S.BAD).all()      # good rows that the flow makes bad
    assert (S.query(v, image, q)[0][spoiled] != S.BAD).all()
    # without a target every good row inside is on a ray without a return
    empty, info = S.build(v, np.zeros((0, 3), F))
    assert info == (0, 0, 0) and (empty == S.EMPTY).all()
    code0, _, counts0 = S.query(v, empty, q, f)
    assert counts0[3] == counts0[4] == counts0[5] == 0 and counts0[2] > 500 and counts0[1] == counts[1] and counts0[0] == counts[0]


def test_the_crowded_pixel_is_one_pixel():
    for shape in ((1024, 64), (8, 3)):
        v = S.view(cases.ORIGIN, W=shape[0], H=shape[1])
        pts, perm = cases.one_pixel(v)
        row, col, rho, _, _ = S.pixel(v, pts)
        assert len(pts) == 5000 and len(set(zip(row.tolist(), col.tolist()))) == 1 and row[0] >= 0
        assert (rho == rho.min()).sum() >= 3 and len(np.unique(rho)) < len(rho) and sorted(perm.tolist()) == list(range(5000))
        a, b = S.build(v, pts), S.build(v, pts[perm])
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] == (0, 0, 1) and a[0][0, row[0], col[0]] == rho.min().view(np.uint32)


def test_the_margin_cases_sit_on_the_equalities():
    v = S.view((0, 0, 0))
    found = cases.margins(v)
    assert len(found) == 5
    for target, q in found:
        image, _ = S.build(v, target)
        code, near, _ = S.query(v, image, q)
        n9 = near[0]
        assert (near == n9).all() and abs(float(n9) - float(target[0, 0])) < 1e-4
        rho = np.sqrt(q[:, 0] * q[:, 0])
        thr = v["margin_abs"] + v["margin_rel"] * rho
        assert rho[0] + thr[0] == n9 and rho[1] + thr[1] < n9 and q[1, 0] == np.nextafter(q[0, 0], F(-np.inf))
        assert rho[2] - thr[2] == n9 and rho[3] - thr[3] > n9 and q[3, 0] == np.nextafter(q[2, 0], F(np.inf))
        assert code.tolist() == [S.AT_FIRST_RETURN, S.SEEN_THROUGH, S.AT_FIRST_RETURN, S.BEHIND]
    assert sorted(float(t[0, 0]) // 1 for t, _ in found) == [2, 7, 20, 61, 150]


def test_the_verdict_scene_spoils_four_segments_each_in_its_own_way():
    from icp_flow_amd import utils_eval
    src, flow, labels, dst = cases.verdict()
    assert 2900 <= len(src) <= 3100
    res = sr.residual(src, src, flow, labels, dst, 2.0, utils_eval.RESIDUAL_EDGES)
    report = utils_eval.SegmentResidual.from_table(sr.table18(res), utils_eval.RESIDUAL_EDGES, 2.0)
    worst = report.worst()
    assert sorted(e["label"] for e in worst) == [cases.PULLED, cases.WALLED, cases.FLUNG, cases.UNSEEN]
    v = S.view((0, 0, 0))
    image, _ = S.build(v, dst)
    seen = S.segments(v, image, src, src, flow, labels, res["d2_before"], res["d2_after"], far=utils_eval.RESIDUAL_EDGES[1])
    s = utils_eval.SegmentSight.from_table(seen["table"])
    verdicts = {e["label"]: e["verdict"] for e in s.annotate(worst)}
    assert verdicts == {cases.PULLED: "seen through", cases.WALLED: "lost from view", cases.FLUNG: "lost from view", cases.UNSEEN: "lost from view"}
    at = {label: k for k, label in enumerate(s.labels.tolist())}
    far = s.after.far
    # each by the code its preparation aims at, and every row of the four is far
    assert far[at[cases.PULLED], 2] > 200 and far[at[cases.WALLED], 4] > 200 and far[at[cases.FLUNG], 0] == 220 and far[at[cases.UNSEEN], 1] > 200
    assert all(s.far_rows(at[k]) == 220 for k in (cases.PULLED, cases.WALLED, cases.FLUNG, cases.UNSEEN))
    for label in (0.0, 1.0, 3.0, 5.0, 7.0, 9.0):
        assert s.far_rows(at[label]) == 0 and s.after.codes[at[label], 2] == 0, label      # on their returns, none seen through

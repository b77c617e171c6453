"""CPU-only: the object boxes (icpflow_segment_boxes, icpflow_pair_objects, csrc/boxes.hip; utils_objects).  The numpy
restatement (tests/box_restatement.py) is held against the truth on rectangle outlines of known yaw, the pair objects against
hand-made motions, every tie case is shown to be the tie its name claims, and the two entry points refuse bad arguments with
their codes and messages before any launch -- no GPU is needed for a refusal."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_cases as bc                        # noqa: E402
import box_restatement as br                  # noqa: E402

F = np.float32
E_ARG, E_WORKSPACE, E_LIMIT = -1, -2, -3
DELTA = 0.05


def test_the_library_is_built_from_the_box_sources_and_keeps_its_number():
    from icp_flow_amd import _lib, build
    assert "boxes.hip" in build.SOURCES and "boxes.hpp" in build.HEADERS
    for name in ("icpflow_segment_boxes", "icpflow_segment_boxes_workspace_bytes", "icpflow_pair_objects", "icpflow_pair_objects_default_params"):
        assert name in _lib.SIGNATURES and hasattr(_lib._L, name)
    assert _lib.VERSION == 215 and (_lib.BOX_COLS, _lib.OBJECT_COLS, _lib.OBJECT_COUNTS) == (br.BOX_COLS, br.OBJECT_COLS, 4)
    p = _lib.ObjectParams.defaults()
    assert (p.struct_size, p.seconds, p.min_speed) == (ctypes.sizeof(_lib.ObjectParams), 0.1, 0.5) and ctypes.sizeof(_lib.ObjectParams) == 24


def test_box_directions_are_the_restatements():
    from icp_flow_amd import utils_objects
    for A in (1, 90, 360):
        d = utils_objects.box_directions(A)
        assert d.dtype == F and d.shape == (A, 2) and np.array_equal(d, br.directions(A))
    assert np.array_equal(br.directions(90)[0], [1.0, 0.0])


def _fit(points, dirs=None, delta=DELTA):
    dirs = br.directions(90) if dirs is None else dirs
    order, table = br.cluster_table(points, np.zeros(len(points), F))
    return br.segment_boxes(points, order, table, 1, dirs, delta)[0]


@pytest.mark.parametrize("sides", (4, 2))
def test_the_restatement_finds_the_yaw_and_the_size_of_noise_free_outlines(sides):
    """k within one step (cyclically) of the true yaw mod 90 degrees, du and dv within 2 delta of the length and the width,
    either way round, on every seeded case"""
    cases = bc.truth_cases(200, 20260 + sides, sides)
    off = []
    for j, case in enumerate(cases):
        box = _fit(case["points"])
        steps = bc.cyclic_steps(box[3], case["yaw"])
        du, dv, L, W = box[9], box[10], case["length"], case["width"]
        sized = (abs(du - L) <= 2 * DELTA and abs(dv - W) <= 2 * DELTA) or (abs(du - W) <= 2 * DELTA and abs(dv - L) <= 2 * DELTA)
        if steps > 1.0 or not sized or box[2] != len(case["points"]):
            off.append((j, box[3], case["yaw"] % 90.0, du, dv, L, W))
    assert not off, (len(off), off[:5])


@pytest.mark.parametrize("sides", (4, 2))
def test_a_yaw_on_the_grid_gives_its_direction_exactly(sides):
    for case in bc.truth_cases(60, 777 + sides, sides, on_grid=True):
        box = _fit(case["points"])
        assert box[3] == case["yaw"] % 90.0, (box[3], case["yaw"])
        assert box[4] == len(case["points"])          # every row of a noise-free outline lies on a side


def test_the_box_centre_and_height_of_a_far_cluster():
    """a cluster 3 km out keeps centimetres: the projections are taken from the centroid, not from the origin"""
    p = bc.outline(4.0, 2.0, 20.0, (3000.0, -3000.0), 400)
    box = _fit(p)
    assert box[3] == 20.0 and abs(box[6] - 3000.0) < 2e-3 and abs(box[7] + 3000.0) < 2e-3
    assert (box[8], box[11], box[14], box[15]) == (0.75, 1.5, 0.0, 1.5)
    assert abs(box[9] - 4.0) < 2e-3 and abs(box[10] - 2.0) < 2e-3


def test_a_far_cluster_keeps_the_precision_of_a_near_one():
    """Points with dyadic coordinates 3 km and 6 km out, one direction (0.6, 0.8): x' = x - r_x is exact (the two lie within a
    factor of two), so du and dv carry four roundings of numbers below 8 m, 4 * 2^-24 * 8 = 1.9e-6 m, however far the cluster
    is -- projecting x itself would cost half an ulp of 3000, 1.2e-4 m, per row."""
    rng = np.random.default_rng(4)
    dirs = np.array([[0.6, 0.8]], F)
    c, s = float(dirs[0, 0]), float(dirs[0, 1])
    for centre in ((3000.0, -3000.0), (-4200.0, 4300.0)):
        local = rng.integers(-128, 129, (200, 2)) / 64.0          # within 2 m of the centre, multiples of 1 / 64
        p = np.concatenate([local + centre, np.zeros((200, 1))], axis=1).astype(F)
        assert np.array_equal(p[:, :2].astype(np.float64), local + centre)
        u, v = p[:, 0].astype(np.float64) * c + p[:, 1].astype(np.float64) * s, p[:, 1].astype(np.float64) * c - p[:, 0].astype(np.float64) * s
        box = _fit(p, dirs, 0.1)
        assert abs(box[9] - (u.max() - u.min())) <= 1.9e-6 and abs(box[10] - (v.max() - v.min())) <= 1.9e-6, (box[9], u.max() - u.min())


# ---------------------------------------------------------------------------------------------------------------- tie cases

def _scores(points, dirs, delta):
    order, table = br.cluster_table(points, np.zeros(len(points), F))
    u, v, _ = br.projections(points, order, table[0], len(points), np.asarray(dirs, F))
    return br.scores(u, v, delta)


def test_tie_near_is_a_tie_on_near_that_the_area_decides():
    case = bc.tie_near()
    dirs = br.directions(case["A"])
    *_, area, near = _scores(case["points"], dirs, case["delta"])
    assert (near == 2).all()
    assert int(np.argmin(area)) == case["k"] and (area == area.min()).sum() == 1 and area[0] > area[case["k"]]
    assert _fit(case["points"], dirs, case["delta"])[3] == case["k"]


def test_tie_area_is_an_exact_tie_on_near_and_area_that_the_lower_direction_wins():
    case = bc.tie_area()
    d, p = case["dirs"], case["points"]
    assert d[2, 0].view(np.uint32) == d[1, 1].view(np.uint32) and d[1, 0].view(np.uint32) == d[2, 1].view(np.uint32)
    assert abs(float(d[1, 0]) ** 2 + float(d[1, 1]) ** 2 - 1.0) <= 1e-3
    as_set = lambda a: sorted(map(tuple, a.tolist()))     # noqa: E731
    assert as_set(p) == as_set(p[:, [1, 0, 2]])           # symmetric under x <-> y
    order, table = br.cluster_table(p, np.zeros(len(p), F))
    assert table[0, 3] == 0.0 and table[0, 4] == 0.0
    *_, area, near = _scores(p, d, case["delta"])
    assert (near == len(p)).all()
    assert area[1].view(np.uint32) == area[2].view(np.uint32) and area[1] < area[0]
    assert _fit(p, d, case["delta"])[3] == case["k"]


def test_rows_at_one_point_tie_everywhere_and_direction_0_wins():
    p = np.tile(np.array([[12.5, -3.25, 0.5]], F), (7, 1))
    box = _fit(p, delta=0.0)
    assert (box[2], box[3], box[4], box[5]) == (7, 0, 7, 0.0) and (box[6], box[7], box[8]) == (12.5, -3.25, 0.5)
    assert (box[9], box[10], box[11]) == (0.0, 0.0, 0.0)


def test_segments_without_a_box():
    pts = np.array([[0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [0, np.inf, 0], [5, 5, 5]], F)
    lab = np.array([-1e8, -1.0, 3.0, 3.0, 7.0], F)
    order, table = br.cluster_table(pts, lab)
    table[2, 3:6] = 0.0                                   # (the centroid of a segment of NaN rows: whatever it is, no row is good)
    boxes = br.segment_boxes(pts, order, table, 4, br.directions(90), 0.1)
    assert boxes[:, 0].tolist() == [-1e8, -1.0, 3.0, 7.0] and boxes[:, 1].tolist() == [1, 1, 2, 1]
    assert boxes[:3, 3].tolist() == [-1, -1, -1] and not boxes[:3, [2] + list(range(4, 16))].any()
    assert boxes[3, 2] == 1 and boxes[3, 3] == 0
    assert br.segment_boxes(pts, order, table, -5, br.directions(90), 0.1).shape == (0, 16)
    assert br.segment_boxes(pts, order, table, 4, br.directions(90), 0.1, Lmax=2).shape == (2, 16)


# ------------------------------------------------------------------------------------------------------------- pair objects

def _one_box(du=4.0, dv=2.0, k_deg=0.0, centre=(10.0, 5.0, 1.0), label=3.0, good=50):
    a = np.deg2rad(k_deg)
    row = np.zeros(16)
    row[0:6] = label, good, good, k_deg, good, du * dv
    row[6:9] = centre
    row[9:12] = du, dv, 1.5
    row[12:14] = F(np.cos(a)), F(np.sin(a))
    row[14:16] = centre[2] - 0.75, centre[2] + 0.75
    return row


def _translation(t):
    T = np.eye(4, dtype=F)
    T[0:3, 3] = t
    return T.reshape(16)


def test_a_pure_translation_gives_its_displacement_and_velocity():
    src = _one_box()[None]
    t = np.array([0.5, -0.25, 0.125], F)                 # (dyadic: T c - c is exact)
    out, counts = br.pair_objects(src, 1, None, 0, [[3.0, 9.0]], [_translation(t)], seconds=0.125)
    assert out[0, 0:4].tolist() == [3.0, 9.0, 0, -1] and out[0, 4:7].tolist() == [10.0, 5.0, 1.0]
    assert out[0, 7:10].tolist() == t.tolist() and out[0, 10:13].tolist() == (t / 0.125).tolist()
    assert out[0, 13] == 16.0 + 4.0 and out[0, 14] == 1.0 and out[0, 21] == -1.0 and out[0, 22:24].tolist() == [50, 0]
    assert counts.tolist() == [1, 1, 0, 1]


def test_motion_along_each_axis_gives_its_quadrant_and_a_tie_the_lower_one():
    src = _one_box(k_deg=0.0)[None]                      # e0 = +x, e1 = +y, e2 = -x, e3 = -y
    for m, t in enumerate(([1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0])):
        out, _ = br.pair_objects(src, 1, None, 0, [[3.0, 3.0]], [_translation(t)])
        assert out[0, 15] == m and out[0, 19:21].tolist() == [[1, 0], [0, 1], [-1, 0], [0, -1]][m]
        assert out[0, 16:19].tolist() == ([4.0, 2.0, 1.5] if m % 2 == 0 else [2.0, 4.0, 1.5])
    for t, m in (([1, 1, 0], 0), ([-1, 1, 0], 1), ([-1, -1, 0], 2), ([1, -1, 0], 0)):   # exact ties of two dot products
        out, _ = br.pair_objects(src, 1, None, 0, [[3.0, 3.0]], [_translation(t)])
        assert out[0, 15] == m, (t, out[0, 15])


def test_standing_objects_face_along_their_longer_side():
    for du, dv, m in ((4.0, 2.0, 0), (2.0, 4.0, 1), (3.0, 3.0, 0)):
        out, counts = br.pair_objects(_one_box(du, dv)[None], 1, None, 0, [[3.0, 3.0]], [_translation([0.01, 0.0, 0.0])])
        assert out[0, 14] == 0.0 and out[0, 15] == m and out[0, 16:18].tolist() == [max(du, dv), min(du, dv)]
        assert counts.tolist() == [1, 0, 0, 1]
    out, _ = br.pair_objects(_one_box()[None], 1, None, 0, [[3.0, 3.0]], [_translation([0.0625, 0.0, 0.0])], seconds=0.125, min_speed=0.5)
    assert out[0, 13] == 0.25 and out[0, 14] == 1.0       # 0.0625 m in 0.125 s is exactly 0.5 m/s: `>=`


def test_missing_labels_give_minus_one_and_the_centre_gap_needs_a_destination_box():
    src = np.stack([_one_box(label=-1.0), _one_box(label=3.0), _one_box(label=8.0)])
    src[0, 2:] = 0.0
    src[0, 3] = -1.0
    dst = np.stack([_one_box(label=5.0, centre=(10.5, 5.0, 1.0)), _one_box(label=6.0)])
    dst[1, 2:] = 0.0
    dst[1, 3] = -1.0
    pairs = [[3.0, 5.0], [4.0, 5.0], [-1.0, 5.0], [8.0, 6.0], [8.0, 7.0], [np.nan, 5.0]]
    T = [_translation([0.5, 0.0, 0.0])] * len(pairs)
    out, counts = br.pair_objects(src, 3, dst, 2, pairs, T)
    assert out[:, 2].tolist() == [1, -1, 0, 2, 2, -1] and out[:, 3].tolist() == [0, 0, 0, 1, -1, 0]
    assert out[0, 21] == 0.0 and out[3, 21] == -1.0 and out[4, 21] == -1.0 and out[0, 23] == 50 and out[3, 23] == 0
    assert not out[[1, 2, 5], 4:].any()
    assert counts.tolist() == [3, 3, 2, 1]
    # -0.0 finds the segment of 0.0
    z = _one_box(label=0.0)[None]
    out, _ = br.pair_objects(z, 1, z, 1, np.array([[-0.0, 0.0]], F), [_translation([0, 0, 0])])
    assert out[0, 2:4].tolist() == [0, 0]


# -------------------------------------------------------------------------------------------------------------------- ABI

def _lib_and_fakes():
    from icp_flow_amd import _lib
    return _lib, _lib._L, ctypes.c_void_p(4096)


def _boxes_call(L, one, **over):
    dirs = over.pop("dirs", br.directions(4))
    a = dict(points=one, n=100, order=one, table=one, num=one, Lmax=16, dirs=dirs.ctypes.data_as(ctypes.c_void_p) if dirs is not None else None,
             A=len(dirs) if dirs is not None else 4, delta=0.1, boxes=one, ws=one, ws_bytes=1 << 30)
    a.update(over)
    rc = L.icpflow_segment_boxes(a["points"], a["n"], a["order"], a["table"], a["num"], a["Lmax"], a["dirs"], a["A"], a["delta"], a["boxes"],
                                 a["ws"], ctypes.c_size_t(a["ws_bytes"]), None)
    return rc, L.icpflow_last_error().decode()


def test_segment_boxes_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    bad = br.directions(4).copy()
    bad[2] = (0.8, 0.8)
    nan = br.directions(4).copy()
    nan[1, 0] = np.nan
    for over, code, text in ((dict(n=-1), E_ARG, "negative"), (dict(n=(1 << 29) + 1), E_LIMIT, "at most"), (dict(Lmax=0), E_ARG, "Lmax"),
                             (dict(Lmax=4097), E_LIMIT, "at most 4096"), (dict(A=0), E_ARG, "A = 0"), (dict(A=361), E_ARG, "A = 361"),
                             (dict(delta=-0.1), E_ARG, "delta"), (dict(delta=1e3 + 1), E_ARG, "delta"), (dict(delta=float("nan")), E_ARG, "delta"),
                             (dict(points=None), E_ARG, "null pointer"), (dict(order=None), E_ARG, "null pointer"),
                             (dict(table=None), E_ARG, "null pointer"), (dict(num=None), E_ARG, "null pointer"),
                             (dict(boxes=None), E_ARG, "null pointer"), (dict(dirs=None), E_ARG, "null pointer"),
                             (dict(dirs=bad), E_ARG, "direction 2"), (dict(dirs=nan), E_ARG, "direction 1"),
                             (dict(ws=None), E_WORKSPACE, "icpflow_segment_boxes_workspace_bytes"),
                             (dict(ws_bytes=int(L.icpflow_segment_boxes_workspace_bytes(100, 16, 4)) - 1), E_WORKSPACE, "workspace of"),
                             (dict(ws=ctypes.c_void_p(4096 + 8)), E_ARG, "16-byte")):
        rc, msg = _boxes_call(L, one, **over)
        assert rc == code and text in msg and msg.startswith("icpflow_segment_boxes"), (over, rc, msg)
    assert L.icpflow_segment_boxes_workspace_bytes(-1, 16, 4) == 0 and L.icpflow_segment_boxes_workspace_bytes(10, 4097, 4) == 0
    assert L.icpflow_segment_boxes_workspace_bytes(10, 16, 361) == 0 and L.icpflow_segment_boxes_workspace_bytes(10, 0, 4) == 0


def test_pair_objects_refuses_bad_arguments_before_any_launch():
    _lib, L, one = _lib_and_fakes()
    good = _lib.ObjectParams.defaults()

    def call(**over):
        a = dict(src=one, num_src=one, dst=one, num_dst=one, Lmax=16, pairs=one, P=3, stride=10, T=one, params=good, objects=one, counts=one)
        a.update(over)
        rc = L.icpflow_pair_objects(a["src"], a["num_src"], a["dst"], a["num_dst"], a["Lmax"], a["pairs"], a["P"], a["stride"], a["T"],
                                    ctypes.byref(a["params"]) if a["params"] is not None else None, a["objects"], a["counts"], None)
        return rc, L.icpflow_last_error().decode()

    short = _lib.ObjectParams.defaults()
    short.struct_size = 16
    for over, code, text in ((dict(P=-1), E_ARG, "negative"), (dict(Lmax=0), E_ARG, "Lmax"), (dict(Lmax=4097), E_LIMIT, "at most 4096"),
                             (dict(stride=1), E_ARG, "pair_stride"), (dict(src=None), E_ARG, "null pointer"),
                             (dict(num_src=None), E_ARG, "null pointer"), (dict(params=None), E_ARG, "null pointer"),
                             (dict(objects=None), E_ARG, "null pointer"), (dict(counts=None), E_ARG, "null pointer"),
                             (dict(dst=None), E_ARG, "come together"), (dict(num_dst=None), E_ARG, "come together"),
                             (dict(pairs=None), E_ARG, "no pair rows"), (dict(T=None), E_ARG, "no transforms"),
                             (dict(params=short), E_ARG, "struct_size"),
                             (dict(params=_lib.ObjectParams.defaults(seconds=0.0)), E_ARG, "seconds"),
                             (dict(params=_lib.ObjectParams.defaults(seconds=float("nan"))), E_ARG, "seconds"),
                             (dict(params=_lib.ObjectParams.defaults(min_speed=-1.0)), E_ARG, "min_speed")):
        rc, msg = call(**over)
        assert rc == code and text in msg and msg.startswith("icpflow_pair_objects"), (over, rc, msg)
    assert L.icpflow_pair_objects_default_params(None) == E_ARG


def test_the_workspace_query_is_aligned_and_never_shrinks():
    _lib, L, _ = _lib_and_fakes()
    ns = [0, 1, 2, 63, 1023, 1024, 1025, 4096, 4097, 63276, 126598, 1 << 20, 1 << 29]
    Ls, As = [1, 2, 16, 512, 4095, 4096], [1, 2, 89, 90, 91, 360]
    size = lambda n, Lmax, A: int(L.icpflow_segment_boxes_workspace_bytes(n, Lmax, A))   # noqa: E731
    for Lmax in Ls:
        for A in As:
            sizes = [size(n, Lmax, A) for n in ns]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes), (Lmax, A, sizes)
    for n in ns:
        for A in As:
            sizes = [size(n, Lmax, A) for Lmax in Ls]
            assert sizes == sorted(sizes), (n, A, sizes)
        for Lmax in Ls:
            sizes = [size(n, Lmax, A) for A in As]
            assert sizes == sorted(sizes), (n, Lmax, sizes)
    a256 = lambda b: (b + 255) // 256 * 256              # noqa: E731  (the header's formula)
    for n, Lmax, A in ((63276, 4096, 90), (5, 16, 1), (1 << 29, 4096, 360)):
        C = n // 1024 + min(n, Lmax) + 1
        want = (a256(4 * (Lmax + 1)) + a256(16 * C * A) + a256(8 * C) + a256(4 * C) + a256(16 * Lmax * A) + a256(8 * Lmax) + a256(4 * Lmax)
                + a256(4 * Lmax * A))
        assert size(n, Lmax, A) == want


# ------------------------------------------------------------------------------------------------------------ Python layer

def test_objects_reads_a_table_into_dicts_and_lines():
    from icp_flow_amd import utils_objects
    src = _one_box(k_deg=0.0)[None]
    rows, counts = br.pair_objects(src, 1, None, 0, [[3.0, 9.0], [4.0, 9.0]], [_translation([0.0, 0.25, 0.0])] * 2, seconds=0.1)
    obj = utils_objects.Objects(rows, counts, seconds=0.1, min_speed=0.5)
    assert obj.summary() == dict(objects=1, movers=1, pairs_without_source_segment=1, pairs_without_destination_segment=2, pairs=2)
    listed = obj.as_list()
    assert len(listed) == 1
    e = listed[0]
    assert (e["label_src"], e["label_dst"], e["moving"], e["centre_gap"], e["points_src"]) == (3.0, 9.0, True, None, 50)
    assert e["size"] == [2.0, 4.0, 1.5] and abs(e["yaw"] - np.pi / 2) < 1e-12 and e["speed"] == 2.5
    assert e["velocity"] == [0.0, 2.5, 0.0] and e["centre"] == [10.0, 5.0, 1.0]
    lines = utils_objects.format_objects(listed)
    assert len(lines) == 2 and "3" in lines[1]
    with pytest.raises(RuntimeError, match="no CPU path"):
        import torch
        utils_objects.segment_boxes_device(torch.zeros(4, 3), torch.zeros(4))


def test_the_command_line_knows_the_flags():
    from icp_flow_amd import frame_pairs
    ns = frame_pairs.argument_parser().parse_args(["dir"])
    assert (ns.objects, ns.sweep_seconds, ns.objects_min_speed) == (None, 0.1, 0.5)
    ns = frame_pairs.argument_parser().parse_args(["dir", "--objects", "--sweep-seconds", "0.05", "--objects-min-speed", "1"])
    assert (ns.objects, ns.sweep_seconds, ns.objects_min_speed) == (True, 0.05, 1.0)
    assert frame_pairs.argument_parser().parse_args(["dir", "--objects", "out.jsonl"]).objects == "out.jsonl"

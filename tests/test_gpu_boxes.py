"""GPU: the object boxes (icpflow_segment_boxes, icpflow_pair_objects, csrc/boxes.hip) against their numpy restatement
(tests/box_restatement.py), value for value (np.array_equal: minima, maxima and counts do not depend on the order of the rows,
so no tolerance is needed anywhere), on guarded buffers and an exactly sized, poisoned workspace (tests/box_device.py); then
frame_pairs.frame_objects and run_stream's flag end to end."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_cases as bc                        # noqa: E402
import box_device as bd                       # noqa: E402
import box_restatement as br                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = bd.DEV
F = np.float32


@pytest.fixture(scope="module")
def sizes_cloud():
    """segments of every size at which the chunking changes, shuffled together with ground and noise rows; its cluster table"""
    points, labels = bc.blobs(bc.SIZES, seed=5)
    return points, labels, bd.cluster_table(points, labels, 64)


def test_segments_of_every_chunking_size(sizes_cloud):
    points, labels, table = sizes_cloud
    got, _ = bd.check_boxes(points, table=table, label="sizes")
    assert got[:, 0].tolist() == [-1e8, -1.0] + [float(j) for j in range(len(bc.SIZES))]
    assert got[:2, 3].tolist() == [-1.0, -1.0] and not got[:2, 4:].any() and got[:2, 1].tolist() == [500, 100]
    assert got[2:, 1].tolist() == list(bc.SIZES) and got[2:, 2].tolist() == list(bc.SIZES)
    assert (got[2:, 3] >= 0).all() and (got[2:, 4] >= 1).all() and (got[5:, 4] < got[5:, 2]).any()


@pytest.mark.parametrize("A,delta", [(1, 0.1), (360, 0.1), (90, 0.0), (7, 1e3)])
def test_other_direction_tables_and_deltas(sizes_cloud, A, delta):
    points, labels, table = sizes_cloud
    got, _ = bd.check_boxes(points, table=table, dirs=br.directions(A), delta=delta, label=f"A = {A}, delta = {delta}")
    assert (got[2:, 3] < A).all()
    if delta == 0.0:
        assert (got[2:, 4] >= 1).all()            # the rows ON a side: an extremum is at distance 0 of itself
    if delta == 1e3:
        assert np.array_equal(got[2:, 4], got[2:, 2])


def test_a_rerun_and_a_second_stream_give_the_same_bytes(sizes_cloud):
    points, labels, table = sizes_cloud
    dirs = br.directions(90)
    _, first = bd.run_boxes(points, *table, dirs, 0.1)
    _, again = bd.run_boxes(points, *table, dirs, 0.1)
    side = torch.cuda.Stream(DEV)
    _, other = bd.run_boxes(points, *table, dirs, 0.1, stream=side)
    assert first == again and first == other


def test_4096_labels_fill_the_table_and_4097_write_nothing():
    rng = np.random.default_rng(11)
    counts = rng.integers(1, 4, 4097)
    labels = np.repeat(np.arange(4097, dtype=F), counts)
    points = (rng.uniform(-50, 50, (4097, 3))[labels.astype(int)] + rng.uniform(-1, 1, (len(labels), 3))).astype(F)
    mix = rng.permutation(len(labels))
    points, labels = points[mix], labels[mix]
    keep = labels < 4096
    got, _ = bd.check_boxes(points[keep], labels[keep], Lmax=4096, label="4096 labels")
    assert len(got) == 4096 and np.array_equal(got[:, 1], counts[:4096]) and (got[:, 3] >= 0).all()
    order, table, num = bd.cluster_table(points, labels, 4096)
    assert int(num.item()) < 0                                    # overflow is the negative count
    got, _ = bd.run_boxes(points, order, table, num, br.directions(90), 0.1)
    assert got.shape == (0, 16)


def test_degenerate_and_far_segments():
    """rows at one point, collinear rows, the `near` tie, rows with NaN / inf coordinates beside good ones and a segment made
    only of them, a cluster 3 km and one 6 km from the origin"""
    tie = bc.tie_near()
    t = np.linspace(-3.0, 3.0, 41)
    line = np.stack([20.0 + t * np.cos(0.3), -7.0 + t * np.sin(0.3), 0.1 * t], axis=1)
    mixed = bc.outline(4.0, 2.0, 33.0, (30.0, 30.0), 80)
    mixed[[3, 17, 40]] = [[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]]
    parts = [np.tile(np.array([[12.5, -3.25, 0.5]], F), (70, 1)), line, tie["points"], mixed, np.full((5, 3), np.nan),
             bc.outline(4.5, 1.9, 61.0, (3000.0, -100.0), 300, sides=2), bc.outline(3.0, 1.5, 12.0, (-4200.0, 4300.0), 1500)]
    points = np.concatenate(parts).astype(F)
    labels = np.concatenate([np.full(len(p), float(j), F) for j, p in enumerate(parts)])
    got, _ = bd.check_boxes(points, labels, label="degenerate")
    assert got[0, 2:6].tolist() == [70, 0, 70, 0.0] and np.abs(got[0, 6:9] - [12.5, -3.25, 0.5]).max() < 1e-5 and not got[0, 9:12].any()
    assert got[1, 4] == 41 and got[1, 3] in (17, 18)               # 0.3 rad is 17.2 degrees
    assert got[2, 3] == tie["k"] and got[2, 4] == 2
    assert got[3, 1] == 80 and got[3, 2] == 77                    # (the three bad rows: their segment's centroid is not finite either)
    assert got[4, 1:4].tolist() == [5, 0, -1]
    for row, (yaw, L, W, c) in ((5, (61.0, 4.5, 1.9, (3000.0, -100.0))), (6, (12.0, 3.0, 1.5, (-4200.0, 4300.0)))):
        assert bc.cyclic_steps(got[row, 3], yaw) <= 1.0, (row, got[row, 3])
        assert sorted([abs(got[row, 9] - L), abs(got[row, 10] - W)])[1] < 0.2 or sorted([abs(got[row, 9] - W), abs(got[row, 10] - L)])[1] < 0.2
        assert abs(got[row, 6] - c[0]) < 0.6 and abs(got[row, 7] - c[1]) < 0.6


def test_the_area_tie_goes_to_the_lower_direction():
    case = bc.tie_area()
    got, _ = bd.check_boxes(case["points"], np.zeros(len(case["points"]), F), dirs=case["dirs"], delta=case["delta"], label="tie_area")
    assert got[0, 3] == case["k"] and got[0, 4] == len(case["points"])
    # the same rows in another order: the same box
    again, _ = bd.check_boxes(case["points"][::-1].copy(), np.zeros(len(case["points"]), F), dirs=case["dirs"], delta=case["delta"])
    assert np.array_equal(got, again)


def test_a_table_that_claims_more_than_the_cloud_holds_is_clipped():
    """a hand-made table: an order entry below 0, one at n and one far beyond; a start + count beyond n; a start beyond n; a
    negative start; a NaN count -- skipped, the guards intact, the restatement's boxes"""
    points, labels = bc.blobs((300, 1500, 40), seed=9, ground=0, noise=0)
    n = len(points)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    order[[5, 250, 400, 1700]] = [-1, n, 1 << 40, -(1 << 33)]
    mean = lambda j: points[labels == j].astype(np.float64).mean(axis=0).astype(F)   # noqa: E731
    table = np.zeros((8, 9))
    table[0, :6] = 0.0, 300, 0, *mean(0)
    table[1, :6] = 1.0, 1500, 300, *mean(1)
    table[2, :6] = 2.0, 5000, 1800, *mean(2)                       # start + count beyond n: cut at n
    table[3, :6] = 3.0, 10, n + 1, *mean(2)                        # a start beyond n
    table[4, :6] = 4.0, 10, -3, *mean(2)                           # a negative start
    table[5, :6] = 5.0, np.nan, 0, *mean(0)                        # a NaN count
    table[6, :6] = 6.0, 1e300, 1790, *mean(2)                      # an absurd count
    table[7, :6] = 7.0, 3e9, 2e9, *mean(2)                         # beyond an int
    dev = (bd.upload(order, np.int64), bd.upload(table, np.float64), bd.upload(np.array([8]), np.int32))
    got, _ = bd.check_boxes(points, table=dev, label="hand-made")
    assert got[:, 2].tolist() == [298, 1498, 40, 0, 0, 0, 50, 0]
    assert np.array_equal(got[:, 1], table[:, 1], equal_nan=True) and got[[3, 4, 5, 7], 3].tolist() == [-1, -1, -1, -1]
    # *d_num above Lmax is read as Lmax
    dev = (dev[0], dev[1], bd.upload(np.array([4000]), np.int32))
    got, _ = bd.run_boxes(points, *dev, br.directions(90), 0.1)
    assert len(got) == 8


# ---- pair objects ---------------------------------------------------------------------------------------------------------------
def _rigid(rng, span=1.0, turn=0.1):
    a = rng.uniform(-turn, turn)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = rng.uniform(-span, span, 3)
    return T.astype(F).reshape(16)


@pytest.mark.parametrize("P", [0, 1, 257])
def test_pair_objects_against_the_restatement(sizes_cloud, P):
    points, labels, table = sizes_cloud
    src, _ = bd.run_boxes(points, *table, br.directions(90), 0.1)
    moved = points + np.array([0.4, -0.2, 0.0], F)
    dst, _ = bd.check_boxes(moved, labels, label="moved")
    rng = np.random.default_rng(P)
    pool = np.array([-1e8, -1.0, -0.0, 0.0, 77.0, 0.5, np.nan] + [float(j) for j in range(len(bc.SIZES))], F)
    pairs = np.zeros((P, 10), F)
    pairs[:, 0], pairs[:, 1] = pool[rng.integers(0, len(pool), P)], pool[rng.integers(0, len(pool), P)]
    pairs[:, 2:] = rng.uniform(-1, 1, (P, 8))
    # (every third pair a translation of centimetres: a standing object)
    T = np.stack([_rigid(rng, 0.02, 0.0) if j % 3 == 0 else _rigid(rng) for j in range(P)]) if P else np.zeros((0, 16), F)
    for tables in ((dst, len(dst)), (None, 0)):
        got, counts = bd.check_objects(src, len(src), tables[0], tables[1], pairs, T, label=f"P = {P}")
        assert counts[0] == (got[:, 22] > 0).sum() and counts[1] == got[:, 14].sum() and counts[2] == (got[:, 2] < 0).sum()
        assert counts[3] == (got[:, 3] < 0).sum() == (P if tables[0] is None else (got[:, 3] < 0).sum())
        assert counts[0] + (got[:, 2] < 0).sum() + ((got[:, 2] >= 0) & (got[:, 22] == 0)).sum() == P
    if P == 257:
        zero = pairs[:, 0] == 0.0                                  # -0.0 and +0.0: the segment of label 0
        assert zero.any() and (np.signbit(pairs[zero, 0])).any() and (got[zero, 2] == 2).all()
        assert (got[np.isnan(pairs[:, 0]), 2] == -1).all() and np.isnan(got[np.isnan(pairs[:, 0]), 0]).all()
        assert (got[:, 14] == 1).any() and ((got[:, 14] == 0) & (got[:, 22] > 0)).any() and set(got[got[:, 22] > 0, 15].tolist()) == {0, 1, 2, 3}
    # other parameters
    if P == 257:
        bd.check_objects(src, len(src), dst, len(dst), pairs, T, seconds=0.5, min_speed=0.0, label="seconds")
        # the destination moved by the pairs' own translation: the centre gap of a segment matched with itself is small
        same = np.stack([np.full(16, j, F) for j in range(len(bc.SIZES))])[:, :2]
        shift = np.eye(4, dtype=F)
        shift[:3, 3] = [0.4, -0.2, 0.0]
        got, _ = bd.check_objects(src, len(src), dst, len(dst), same, np.tile(shift.reshape(16), (len(same), 1)), label="self")
        assert (got[:, 21] >= 0).all() and np.median(got[:, 21]) < 0.1 ** 2, got[:, 21]


def test_a_nan_label_finds_the_segment_with_its_bits():
    boxes = np.zeros((3, 16))
    boxes[:, 0] = 1.0, 2.0, np.nan
    boxes[:, 2:4] = [[5, 0]] * 3
    boxes[:, 6] = 10.0, 20.0, 30.0
    boxes[:, 9:14] = [[2, 1, 1, 1, 0]] * 3
    T = np.tile(np.eye(4, dtype=F).reshape(16), (3, 1))
    got, counts = bd.check_objects(boxes, 3, None, 0, np.array([[np.nan, 1.0], [-np.nan, 1.0], [2.0, np.nan]], F), T, label="nan")
    assert got[:, 2].tolist() == [2, -1, 1] and got[0, 4] == 30.0 and counts.tolist() == [2, 0, 1, 3]


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def registered():
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_frame_pair(seed=2, n_objects=8, n_max=600, n_background=1500)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], gt_flow=d["gt_flow"], name="synthetic")
    a = frame_pairs.default_args()
    a.objects = True
    out = frame_pairs.register_frame_pair(a, fp, DEV)
    return fp, out


def test_frame_objects_equals_the_restatement_on_what_the_registration_left(registered):
    from icp_flow_amd import _lib, frame_pairs, utils_objects
    fp, out = registered
    objects = frame_pairs.frame_objects(fp, out, DEV)
    pairs, T = out["pairs"].cpu().numpy(), out["transformations"].cpu().numpy()
    assert len(pairs) >= 4 and objects.rows.shape == (len(pairs), 24) and objects.seconds == 0.1
    tables = []
    for pts, lab in ((fp.points_src, fp.labels_src), (fp.points_dst, fp.labels_dst)):
        _, order, table, num = utils_objects.cluster_table_device(torch.from_numpy(pts).to(DEV), torch.from_numpy(lab).to(DEV))
        tables.append((br.segment_boxes(pts, order.cpu().numpy(), table.cpu().numpy(), int(num.item()), br.directions(90), 0.1), int(num.item())))
    want, counts = br.pair_objects(tables[0][0], tables[0][1], tables[1][0], tables[1][1], pairs[:, :2], T.reshape(-1, 16), 0.1, 0.5)
    bd.same(objects.rows, want, "frame_objects")
    assert np.array_equal(objects.counts, counts) and counts[0] == len(pairs) and counts[2] == 0 and counts[3] == 0
    # columns 7 - 9 against icpflow_transform_points applied to the centre: four roundings per component of the float32 kernel,
    # |got - exact| <= 5 u (|R| |c| + |t|), the bound of COVERAGE.md row a-10
    c = objects.rows[:, 4:7]
    x = torch.zeros((len(pairs), 1, 4), dtype=torch.float32, device=DEV)
    x[:, 0, :3] = torch.from_numpy(c.astype(F)).to(DEV)
    moved = torch.empty_like(x)
    _lib.call("icpflow_transform_points", _lib.ptr(x), _lib.ptr(out["transformations"].float().contiguous()), len(pairs), 1, _lib.ptr(moved), _lib.stream(DEV))
    d32 = moved[:, 0, :3].cpu().numpy().astype(np.float64) - c
    R, t = np.abs(T[:, :3, :3].astype(np.float64)), np.abs(T[:, :3, 3].astype(np.float64))
    bound = 5 * 2.0 ** -24 * (np.einsum("pij,pj->pi", R, np.abs(c)) + t)
    ratio = np.abs(objects.rows[:, 7:10] - d32) / bound
    print(f"max |d - (transform_points(c) - c)| / bound = {ratio.max():.3f}")
    assert (ratio <= 1.0).all(), float(ratio.max())
    # what the objects say: every pair has a box on either side
    listed = objects.as_list()
    assert len(listed) == len(pairs) and all(e["centre_gap"] is not None and e["points_src"] > 0 and e["points_dst"] > 0 for e in listed)
    assert objects.largest_centre_gap() == max(e["centre_gap"] for e in listed)
    assert len(utils_objects.format_objects(listed)) == len(pairs) + 1


def test_run_stream_writes_the_file_and_leaves_the_summary_alone(registered, tmp_path):
    from icp_flow_amd import frame_pairs
    fp, _ = registered
    a = frame_pairs.default_args()
    plain = frame_pairs.run_stream(a, [fp, fp], DEV)
    path = str(tmp_path / "objects.jsonl")
    b = SimpleNamespace(**vars(a))
    b.objects, b.sweep_seconds, b.objects_min_speed = path, 0.05, 1.0
    s = frame_pairs.run_stream(b, [fp, fp], DEV)
    assert [k for k in s if k not in plain] == ["objects", "ms_objects_per_frame_pair", "objects_file"] and s["ms_objects_per_frame_pair"] > 0
    timing = ("ms_per_frame_pair", "frame_pairs_per_s")
    assert {k: v for k, v in s.items() if k in plain and k not in timing} == {k: v for k, v in plain.items() if k not in timing}
    lines = [json.loads(line) for line in open(path)]
    assert len(lines) == 2 and [e["frame_pair"] for e in lines] == [0, 1] and lines[0]["objects"] == lines[1]["objects"]
    assert lines[0]["seconds"] == 0.05 and lines[0]["counts"]["pairs"] == s["matched_cluster_pairs"] // 2
    block = s["objects"]
    assert block["objects"] == sum(e["counts"]["objects"] for e in lines) and block["movers"] == sum(e["counts"]["movers"] for e in lines)
    assert block["pairs_without_box"] == 0 and block["sweep_seconds"] == 0.05 and block["min_speed"] == 1.0
    assert abs(block["largest_centre_gap"] - max(o["centre_gap"] for e in lines for o in e["objects"])) < 1e-12
    assert set(lines[0]["objects"][0]) == {"pair", "label_src", "label_dst", "centre", "size", "yaw", "velocity", "speed", "moving", "centre_gap",
                                           "points_src", "points_dst"}
    c = frame_pairs.default_args()
    c.objects = True                                               # bare: no file
    assert "objects_file" not in frame_pairs.run_stream(c, [fp], DEV)

"""icpflow_nn_residual_segments on the GPU against the numpy restatement (tests/segment_residual_restatement.py, checked on a
hand-counted scene in tests/test_segment_residual.py): label, rows and every count equal, each sum within (rows - 1) 2^-53 sum
of math.fsum, the per-row d2 of both sides bit for bit and equal to two icpflow_nn_residual calls; every output between guards,
the workspace of exactly the queried size filled with 0xFF (tests/segment_residual_device.py).  Segment sizes over the wave,
workgroup and chunk edges; Lmax labels and one more; the label rules; rows bad on one side; every pointer variant; ties and
d2 == r2; a crowded cell; reruns and streams; the group table of icpflow_nn_residual as a cross-check; the verdict on a spoiled
flow; and run_stream end to end.  The scenes' own conditions are asserted on the CPU (tests/test_segment_residual.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_device as rd                  # noqa: E402
import segment_residual_cases as cases        # noqa: E402
import segment_residual_device as sd          # noqa: E402
import segment_residual_restatement as sr     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = sd.DEV
EDGES = cases.EDGES


# ---- shapes -----------------------------------------------------------------------------------------------------------------
def test_segment_sizes_over_the_wave_workgroup_and_chunk_edges_in_one_cloud():
    b, a, f, lab, t = sd.scene(cases.SEGMENT_SIZES, 3000, seed=3)
    got, want = sd.check(b, a, f, lab, t, 1.0, EDGES, label="segment sizes")
    assert got["table"][:, 1].tolist() == list(cases.SEGMENT_SIZES)
    assert 0 < int(want["before"]["hits"].sum()) < len(b) and int(got["info"][3]) > 100
    # the per-row outputs are what two icpflow_nn_residual calls write
    for key, query, flow in (("d2_before", b, None), ("d2_after", a, f)):
        alone = rd.run(query, t, flow, 1.0, outputs=("d2",))
        assert np.array_equal(got[key].view(np.int32), alone["d2"].view(np.int32)), key


@pytest.mark.parametrize("n", (0, 1, 2049))
def test_empty_single_and_odd_clouds(n):
    for m in (0, 1, 2049):
        sizes = () if n == 0 else (n,) if n == 1 else (700, 1, 1348)
        b, a, f, lab, t = sd.scene(sizes, m, seed=100 + n + m, span=3.0)
        got, want = sd.check(b, a, f, lab, t, 1.0, EDGES, label=f"{n} x {m}")
        assert got["num"] == len(sizes)
        if m == 0 and n:
            assert (got["table"][:, 3] == 0).all() and (got["table"][:, 11] == 0).all() and (got["d2_after"] == 1.0).all()   # every good query a miss


@pytest.mark.parametrize("Lmax", (4, 4096))
def test_lmax_labels_exactly_and_one_more(Lmax):
    rng = np.random.default_rng(Lmax)
    t = rng.uniform(-3, 3, (500, 3)).astype(np.float32)
    for L in (Lmax, Lmax + 1):
        n = L + 40
        lab = np.concatenate([np.arange(L), rng.integers(0, L, 40)]).astype(np.float32)[rng.permutation(n)]
        b = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
        f = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
        if L == Lmax:
            got, _ = sd.check(b, b, f, lab, t, 1.0, EDGES, Lmax, same_after=True, label=f"{L} labels, Lmax {Lmax}")
            assert got["num"] == Lmax
        else:       # the negative count, and nothing of the table written (sd.run asserts the poison); the rows are still judged
            got = sd.run(b, b, f, lab, t, 1.0, EDGES, Lmax, same_after=True)
            assert got["num"] == -(Lmax + 1) and got["table"].shape == (0, 18)
            want = sr.residual(b, b, f, lab, t, 1.0, EDGES)
            assert np.array_equal(got["d2_after"], want["d2_after"]) and tuple(got["info"][:3]) == want["info"]


def test_label_values():
    lab, L = cases.label_values()
    rng = np.random.default_rng(6)
    b = rng.uniform(-2, 2, (len(lab), 3)).astype(np.float32)
    t = rng.uniform(-2, 2, (50, 3)).astype(np.float32)
    got, want = sd.check(b, b, None, lab, t, 1.0, EDGES, same_after=True, label="label values")
    assert got["num"] == L and got["table"][:5, 0].tolist() == [-1e8, -1.0, 0.0, 3.0, 7.0] and np.isnan(got["table"][5, 0])
    assert not np.signbit(got["table"][2, 0]) and got["table"][:, 1].tolist() == [2, 2, 4, 2, 1, 2]
    # NaN labels of several bit patterns, either sign: one segment each, negative NaNs first, positive NaNs last
    nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    lab2 = np.concatenate([nans, np.array([np.inf, -np.inf, 1.0], np.float32)])
    got, want = sd.check(b[:9], b[:9], None, lab2, t, 1.0, (), same_after=True, label="NaN labels")
    assert got["num"] == 7 and np.isnan(got["table"][[0, 4, 5, 6], 0]).all() and got["table"][1:4, 0].tolist() == [-np.inf, 1.0, np.inf]


# ---- rows and arguments -----------------------------------------------------------------------------------------------------
def test_rows_bad_on_one_side_only():
    before, after, flow, labels, target, inf_rows, pad_src, pad_dst = cases.one_side_bad()
    got, want = sd.check(before, after, flow, labels, target, 1.0, EDGES, label="one side bad")
    assert got["info"][:3].tolist() == [len(pad_src), len(pad_src) + len(inf_rows), len(pad_dst)]
    assert int(got["table"][:, 2].sum()) == len(before) - len(pad_src)
    assert int(got["table"][:, 10].sum()) == len(before) - len(pad_src) - len(inf_rows)
    assert int(got["table"][:, 1].sum()) == len(before)
    r2 = np.float32(1.0)
    assert (got["d2_after"][inf_rows] == r2).all() and (got["d2_before"][pad_src] == r2).all()
    # every target a pad row: nothing in the grid, every good query a miss
    got, _ = sd.check(before, after, flow, labels, np.full((40, 3), 1e8, np.float32), 1.0, EDGES, label="pads only")
    assert got["info"][2:5].tolist() == [40, 0, 0] and (got["table"][:, 3] == 0).all() and (got["table"][:, 11] == 0).all()


def test_pointer_variants():
    b, a, f, lab, t = sd.scene((300, 500, 77), 900, seed=23, span=4.0)
    full, _ = sd.check(b, a, f, lab, t, 1.0, EDGES, label="all")
    for outputs in (("d2_before",), ("d2_after",), ()):                        # each optional output NULL in turn, and both
        got, _ = sd.check(b, a, f, lab, t, 1.0, EDGES, outputs=outputs, label=f"outputs {outputs}")
        assert got["table"].tobytes() == full["table"].tobytes() and got["info"].tobytes() == full["info"].tobytes()
        for k in outputs:
            assert got[k].tobytes() == full[k].tobytes(), k
    got, _ = sd.check(b, a, None, lab, t, 1.0, EDGES, label="no flow")         # q = d_after
    assert got["table"][:, 2:10].tobytes() == full["table"][:, 2:10].tobytes()
    same, _ = sd.check(b, b, f, lab, t, 1.0, EDGES, same_after=True, label="d_after == d_before")
    copy, _ = sd.check(b, b.copy(), f, lab, t, 1.0, EDGES, label="d_after a copy of d_before")
    assert same["table"].tobytes() == copy["table"].tobytes() and same["d2_after"].tobytes() == copy["d2_after"].tobytes()
    still, _ = sd.check(b, b, None, lab, t, 1.0, EDGES, same_after=True, label="nothing moves")
    assert still["table"][:, 2:10].tobytes() == still["table"][:, 10:18].tobytes()
    sd.run(b, a, f, lab, t, 1.0, EDGES, short=1, expect=-2, expect_message="icpflow_nn_residual_segments_workspace_bytes")
    sd.run(b, a, f, lab, t, 1.0, (0.1, 0.05), expect=-1, expect_message="edges")
    sd.run(b, a, f, lab, t, 1.0, EDGES, Lmax=4097, expect=-3, expect_message="at most 4096 segments")


def test_no_edges_and_four():
    b, a, f, lab, t = sd.scene((300, 500, 77), 900, seed=24, span=4.0)
    none, _ = sd.check(b, a, f, lab, t, 1.0, (), label="E = 0")
    four, want = sd.check(b, a, f, lab, t, 1.0, (0.1, 0.3, 0.6, 1.0), label="E = 4")
    assert (none["table"][:, [4, 5, 6, 7, 12, 13, 14, 15]] == 0).all()
    assert (four["table"][:, 7] == four["table"][:, 2]).all() and (four["table"][:, 15] == four["table"][:, 10]).all()   # an edge at the radius: every good row
    assert four["table"][:, [8, 9, 16, 17]].tobytes() == none["table"][:, [8, 9, 16, 17]].tobytes()
    assert 0 < four["table"][:, 5].sum() < four["table"][:, 6].sum() < four["table"][:, 7].sum()


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_ties_and_d2_equal_to_r2_on_a_lattice():
    before, after, flow, labels, target, radius = cases.lattice()
    got, want = sd.check(before, after, flow, labels, target, radius, EDGES, label="lattice")
    r2 = np.float32(radius) * np.float32(radius)
    for side, at in (("d2_before", 2), ("d2_after", 10)):
        assert int((got[side] == r2).sum()) == 150
        assert got["table"][:, at].sum() == 300 and got["table"][:, at + 1].sum() == 300       # d2 == r2 is a hit, on either side
        assert sorted(set(got[side].tolist())) == [0.0625, 0.25]


def test_five_thousand_targets_in_one_cell():
    before, after, flow, labels, target, radius = cases.one_cell()
    got, _ = sd.check(before, after, flow, labels, target, radius, EDGES, label="one cell")
    assert got["info"][3:5].tolist() == [1, 5000]


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_reruns_and_streams_give_identical_bits():
    """crowded buckets (the scatter's order inside a bucket is whatever the atomics made it), segments of several chunks"""
    b, a, f, lab, t = sd.scene((2500, 3000, 500), 5000, seed=31, span=3.0)
    first, _ = sd.check(b, a, f, lab, t, 1.0, EDGES, label="first")
    runs = [sd.run(b, a, f, lab, t, 1.0, EDGES, ws_poison=p) for p in (0x00, 0xA5)]
    for s in (torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)):
        with torch.cuda.stream(s):
            runs.append(sd.run(b, a, f, lab, t, 1.0, EDGES))
    for other in runs:
        for k in ("table", "d2_before", "d2_after", "info"):
            assert other[k].tobytes() == first[k].tobytes(), k
    assert int(first["info"][4]) >= 4


# ---- against the group table ------------------------------------------------------------------------------------------------
def test_the_segments_of_a_group_add_up_to_the_group_tables_words():
    from icp_flow_amd import frame_pairs
    before, after, flow, labels, target = cases.verdict()
    pairs = torch.zeros((3, 10))
    pairs[:, 0] = torch.tensor([0.0, 2.0, 5.0])
    groups = frame_pairs.residual_groups(torch.from_numpy(labels), pairs).numpy()
    got = sd.run(before, after, flow, labels, target, 2.0, EDGES)
    seg_group = frame_pairs.residual_groups(torch.from_numpy(got["table"][:, 0].astype(np.float32)), pairs).numpy()
    assert sorted(set(seg_group.tolist())) == [0, 1, 2, 3]
    E = len(EDGES)
    for at, query, f in ((2, before, None), (10, after, flow)):
        words = rd.run(query, target, f, 2.0, groups, 4, EDGES, outputs=("table",))["words"].reshape(4, E + 4)
        for g in range(4):
            mine = got["table"][seg_group == g]
            assert mine[:, at: at + 2 + E].sum(axis=0).tolist() == words[g, : 2 + E].tolist(), (at, g)


# ---- the verdict ------------------------------------------------------------------------------------------------------------
def test_a_spoiled_segment_is_the_one_listed():
    from icp_flow_amd import utils_eval
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)   # noqa: E731
    before, after, flow, labels, target = cases.verdict(sabotage=True)
    pairs = torch.zeros((2, 10))
    pairs[0, :2], pairs[1, :2] = torch.tensor([cases.SABOTAGED, 17.0]), torch.tensor([4.0, 4.0])
    pb = up(before)
    report = utils_eval.segment_residual(pb, pb, up(flow), up(labels), up(target), radius=2.0)
    assert len(report) == 8 and report.labels.tolist() == [-1e8, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert report.rows.sum() == len(before) and report.info["bad_queries_after"] == 0 and report.info["longest_bucket"] >= 1
    worst = report.worst(pairs=pairs)
    assert [e["label"] for e in worst] == [cases.SABOTAGED]
    e = worst[0]
    assert e["gain"] < 0 and e["after_mean"] > 0.1 and e["matched"] and e["pair"] == [cases.SABOTAGED, 17.0]
    assert e["rows"] == int((labels == cases.SABOTAGED).sum()) and 0.0 <= e["hit_rate_after"] <= 1.0
    assert utils_eval.format_segment_residual(worst)[0].startswith("residual segment:   2, after: ")
    # the device form reads nothing back and fills the per-row arrays on request
    table, num, info, d2b, d2a = utils_eval.segment_residual_device(pb, pb, up(flow), up(labels), up(target), 2.0, Lmax=64, per_row=True)
    assert table.shape == (64, 18) and table.is_cuda and int(num) == 8 and info.shape == (6,) and d2b.shape == d2a.shape == (len(before),)
    assert float(d2a[up(labels) == cases.SABOTAGED].mean()) > 0.01
    with pytest.raises(ValueError, match="distinct labels"):
        utils_eval.segment_residual(pb, pb, up(flow), up(labels), up(target), radius=2.0, Lmax=7)
    # unsabotaged: nothing to list
    before, after, flow, labels, target = cases.verdict(sabotage=False)
    clean = utils_eval.segment_residual(up(before), up(after), up(flow), up(labels), up(target), radius=2.0)
    assert clean.worst(pairs=pairs) == [] and (clean.gain()[2:] > 0).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------
LOST = 1.0      # the object the destination frame does not see: its segment stays where the ego pose left it


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    from icp_flow_amd import frame_pairs
    root = tmp_path_factory.mktemp("segments")
    for seed in (41, 42, 43):
        d = cases.rigid_pair(seed)
        seen = d["labels_src"] != LOST
        fp = frame_pairs.FramePair(d["points_src"], d["points_dst"][seen], d["labels_src"], d["labels_src"][seen], d["pose"], name=f"rigid_{seed}")
        frame_pairs.save_frame_pair(str(root / f"fp_{seed}.npz"), fp)
    return str(root)


def test_run_stream_with_the_attribute(directory, tmp_path):
    from icp_flow_amd import frame_pairs
    paths = frame_pairs.list_frame_pairs(directory)
    a = frame_pairs.default_args(max_points=2048)
    a.residual = 2.0
    plain = frame_pairs.run_stream(a, paths, DEV)
    assert "residual_segments" not in plain and "ms_segment_residual_per_frame_pair" not in plain
    a.residual_segments = True
    blocks = {}
    for in_flight in (1, 4):
        s = frame_pairs.run_stream(a, paths, DEV, in_flight=in_flight)
        assert [k for k in s if k not in plain] == ["residual_segments", "ms_segment_residual_per_frame_pair"]
        assert s["ms_segment_residual_per_frame_pair"] > 0
        assert json.dumps(s["residual"], sort_keys=True) == json.dumps(plain["residual"], sort_keys=True)
        blocks[in_flight] = json.dumps(s["residual_segments"], sort_keys=True)
    assert blocks[1] == blocks[4]
    block = json.loads(blocks[1])
    assert sorted(block) == ["above", "segments_judged", "segments_listed", "worst"]
    assert block["above"] == 0.1 and block["segments_judged"] == 18 and block["segments_listed"] == len(block["worst"]) >= 3
    lost = [e for e in block["worst"] if e["label"] == LOST]
    assert sorted(e["frame_pair"] for e in lost) == [0, 1, 2] and not any(e["matched"] for e in lost)
    assert sorted(e["path"] for e in lost) == ["fp_41.npz", "fp_42.npz", "fp_43.npz"]
    means = [e["after_mean"] for e in block["worst"]]
    assert means == sorted(means, reverse=True) and min(means) > 0.1
    # a file name: the whole list as JSON
    a.residual_segments = str(tmp_path / "worst.json")
    s = frame_pairs.run_stream(a, paths, DEV)
    assert s["residual_segments_file"] == a.residual_segments and json.load(open(a.residual_segments)) == block["worst"]


def test_the_command_line_writes_the_file(directory, tmp_path, capsys):
    from icp_flow_amd import frame_pairs
    out = str(tmp_path / "cli.json")
    frame_pairs.main([directory, "--max-points", "2048", "--residual", "--residual-segments", out])
    text = capsys.readouterr().out
    listed = json.load(open(out))
    assert "residual segment: frame pair:" in text and any(e["label"] == LOST for e in listed)
    summary = json.loads(text.strip().splitlines()[-1])
    assert summary["residual_segments_file"] == out and summary["residual_segments"]["segments_listed"] == len(listed)

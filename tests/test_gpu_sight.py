"""GPU: the line-of-sight check (icpflow_sight_build / _query / _segments, csrc/sight.hip) against its numpy restatement
(tests/sight_restatement.py), array_equal throughout -- the map uses no transcendental function, so every bit of the image, every
code and every count is a function of the arguments alone.  Every call runs on guarded, poisoned buffers and a 0xFF workspace of
exactly the queried size (tests/sight_device.py); the scenes' own conditions are asserted on the CPU (tests/test_sight.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_residual_cases as rcases       # noqa: E402
import segment_residual_device as rsd         # noqa: E402
import sight_cases as cases                   # noqa: E402
import sight_device as sd                     # noqa: E402
import sight_restatement as S                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = sd.DEV
F = np.float32


# ---- the image ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0, 0, 0), cases.ORIGIN], ids=["o0", "o1"])
@pytest.mark.parametrize("shape", cases.SHAPES, ids=[f"{W}x{H}" for W, H in cases.SHAPES])
def test_image_shapes_and_the_borders_of_the_map(shape, origin):
    """columns 0 and W - 1 (the wrap of the 3 x 3 pass), p rounding to 4, rows 0 and H - 1 (the clip), t == tan_lo and the float
    below tan_hi, rho on either bound and beside it, the vertical axis, a non-zero origin; then a sweep all around"""
    W, H = shape
    v = S.view(origin, W=W, H=H)
    border = np.stack([p for _, p in cases.border_points(v)])
    sd.check_frame(border, border, None, origin, label="borders", W=W, H=H)
    target = np.concatenate([border, cases.sweep(700, 5 + W + H, v, bad=True)])
    q, f, _ = cases.queries(900, 9 + W + H, v, target, bad=True)
    got, seen, _ = sd.check_frame(target, np.concatenate([q, border]), np.concatenate([f, np.zeros_like(border)]), origin, label="sweep", W=W, H=H)
    assert got["info"][2] > 0 and (seen["counts"] > 0).sum() >= 4


def test_five_thousand_targets_in_one_pixel_in_two_row_orders():
    """atomicMin: duplicates, the minimum several times, the same cloud in two orders -- the same image"""
    v = S.view(cases.ORIGIN)
    pts, perm = cases.one_pixel(v)
    a, _, _ = sd.check_frame(pts, pts[:300], None, cases.ORIGIN, label="one pixel")
    b, _, _ = sd.check_frame(pts[perm], pts[:300], None, cases.ORIGIN, label="one pixel, permuted")
    assert a["image"].tobytes() == b["image"].tobytes() and a["info"].tolist() == b["info"].tolist() == [0, 0, 1]


def test_the_margins_decide_at_the_equalities():
    """rho + thr == n9 is not seen through and the float below it is; rho - thr == n9 is at the first return and the float
    above it is behind -- at five ranges (tests/sight_cases.py finds the floats by search)"""
    for target, q in cases.margins(S.view((0, 0, 0))):
        _, seen, _ = sd.check_frame(target, q, None, label=f"margin at {float(target[0, 0]):g}")
        assert seen["code"].tolist() == [S.AT_FIRST_RETURN, S.SEEN_THROUGH, S.AT_FIRST_RETURN, S.BEHIND]


@pytest.mark.parametrize("n", cases.SIZES)
def test_row_counts_over_the_wave_and_the_workgroup(n):
    """n and m over 0 .. 2049 (m runs the other way), NaN, Inf and pad rows on either side, a flow that makes a good row bad,
    no flow, no near output, no target"""
    v = S.view(cases.ORIGIN)
    m = cases.SIZES[len(cases.SIZES) - 1 - cases.SIZES.index(n)]
    target = cases.sweep(m, 100 + m, v, bad=True)
    q, f, spoiled = cases.queries(n, 200 + n, v, target, bad=True)
    got, seen, (image, code) = sd.check_frame(target, q, f, cases.ORIGIN, label=f"n {n} m {m}")
    assert (seen["code"][spoiled] == S.BAD).all()
    sd.check_frame(target, q, None, cases.ORIGIN, label=f"n {n} m {m}, no flow")
    bare = sd.query(image, q, f, cases.ORIGIN, near=False)
    assert np.array_equal(bare["code"], code) and bare["near"] is None
    # m = 0: an empty image, and every good row inside is on a ray without a return
    _, empty, _ = sd.check_frame(target[:0], q, f, cases.ORIGIN, label=f"n {n}, m 0")
    assert empty["counts"][3:].tolist() == [0, 0, 0] and empty["counts"][:2].tolist() == seen["counts"][:2].tolist()


# ---- the segments -------------------------------------------------------------------------------------------------------------
def _scene(sizes, m, seed, labels=None, bad=False, origin=cases.ORIGIN, **view_params):
    """segments of the given sizes shuffled over one cloud, `after` a jittered copy, and the distances of both sides from a
    REAL icpflow_nn_residual_segments call (radius 1)"""
    v = S.view(origin, **view_params)
    n = int(sum(sizes))
    target = cases.sweep(m, seed, v, bad=bad)
    before, flow, _ = cases.queries(n, seed + 1, v, target, bad=bad)
    rng = np.random.default_rng(seed + 2)
    values = np.arange(len(sizes), dtype=F) if labels is None else np.asarray(labels, F)
    lab = np.repeat(values, sizes)[rng.permutation(n)]
    after = (before + rng.normal(0.0, 0.1, before.shape)).astype(F)
    d2 = rsd.run(before, after, flow, lab, target, 1.0, (), max(len(sizes), 1))
    return target, before, after, flow, lab, d2["d2_before"], d2["d2_after"]


def test_segment_sizes_over_the_wave_workgroup_and_chunk_edges_in_one_cloud():
    """1 .. 1025 and 3 * 1024 + 777 rows in one cloud; the per-row codes are the query's; the segments add up to its counts"""
    target, before, after, flow, lab, d2b, d2a = _scene(rcases.SEGMENT_SIZES, 3000, 61, bad=True)
    got, want, image = sd.check_segments(target, before, after, flow, lab, d2b, d2a, far=0.1, origin=cases.ORIGIN, label="sizes")
    assert got["table"][:, 1].tolist() == list(rcases.SEGMENT_SIZES)
    for side, pts, f, at in (("code_before", before, None, 2), ("code_after", after, flow, 13)):
        seen = sd.query(image, pts, f, cases.ORIGIN)
        assert np.array_equal(got[side], seen["code"]), side
        counts = seen["counts"].tolist()
        assert got["info"][6 * (at > 2): 6 * (at > 2) + 6].tolist() == counts
        assert got["table"][:, at + 1: at + 11: 2].sum(axis=0).tolist() == counts[1:]
        assert got["table"][:, at].sum() == sum(counts[1:]) and (got["table"][:, 1] - got["table"][:, at]).sum() == counts[0]
        assert (got["table"][:, at + 2: at + 12: 2] <= got["table"][:, at + 1: at + 11: 2]).all()
    assert got["table"][:, 4:13:2].sum() > 100 and got["table"][:, 15:24:2].sum() > 100          # there ARE far rows
    assert (got["table"][:, 1] > got["table"][:, 13]).any()                                       # and rows bad AFTER only


@pytest.mark.parametrize("n", (0, 1, 2049))
def test_empty_single_and_odd_clouds(n):
    target, before, after, flow, lab, d2b, d2a = _scene((n,) if n else (), 500, 63)
    got, _, _ = sd.check_segments(target, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, label=f"n {n}")
    assert got["num"] == (1 if n else 0)
    sd.check_segments(target[:0], before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, label=f"n {n}, no target")


@pytest.mark.parametrize("Lmax", (4, 4096))
def test_lmax_labels_exactly_and_one_more(Lmax):
    rng = np.random.default_rng(Lmax)
    sizes = rng.integers(1, 4, Lmax)
    target, before, after, flow, lab, d2b, d2a = _scene(sizes, 800, 65 + Lmax, labels=rng.permutation(Lmax).astype(F) - 7)
    got, _, image = sd.check_segments(target, before, after, flow, lab, d2b, d2a, Lmax=Lmax, origin=cases.ORIGIN, label=f"{Lmax} labels")
    assert got["num"] == Lmax
    # one label more: the negative count, no row of the table, no code, zeros in d_info
    more = np.concatenate([lab, [F(Lmax + 100)]])
    grow = lambda x: np.concatenate([x, x[:1]])    # noqa: E731
    over = sd.segments(image, grow(before), grow(after), grow(flow), more, grow(d2b), grow(d2a), Lmax=Lmax, origin=cases.ORIGIN)
    assert over["num"] == -(Lmax + 1) and over["table"].size == 0 and not over["info"].any()
    assert (over["code_before"].view(np.uint8) == 0xA5).all() and (over["code_after"].view(np.uint8) == 0xA5).all()


def test_label_values():
    """both zeros one label, ground and noise labels, a NaN label"""
    lab, L = rcases.label_values()
    v = S.view(cases.ORIGIN)
    target = cases.sweep(400, 71, v)
    before, flow, _ = cases.queries(len(lab), 72, v, target)
    got, want, _ = sd.check_segments(target, before, before, flow, lab, origin=cases.ORIGIN, same_after=True, label="label values")
    assert got["num"] == L and not np.signbit(got["table"][2, 0]) and got["table"][:, 1].tolist() == [2, 2, 4, 2, 1, 2]


def test_rows_bad_on_one_side_only():
    before, after, flow, labels, target, inf_rows, pad_src, pad_dst = rcases.one_side_bad()
    shift = np.array([20.0, 3.0, 0.0], F)              # (the residual's scene sits around the origin: move it into view)
    got, want, _ = sd.check_segments(target + shift, before + shift, after + shift, flow, labels, label="one side bad")
    assert got["info"][0] == len(pad_src) and got["info"][6] == len(pad_src) + len(inf_rows)
    assert (got["code_after"][inf_rows] == S.BAD).all() and (got["code_before"][inf_rows] != S.BAD).all()
    assert (got["table"][:, 2] > got["table"][:, 13]).any()


def test_every_optional_pointer_null_in_turn():
    target, before, after, flow, lab, d2b, d2a = _scene((700, 300, 1200), 1500, 75, bad=True)
    full, _, image = sd.check_segments(target, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, label="all given")
    for outputs in (("code_before",), ("code_after",), ()):
        got, _, _ = sd.check_segments(target, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, outputs=outputs, label=str(outputs))
        assert got["table"].tobytes() == full["table"].tobytes()
    for b2, a2 in ((None, d2a), (d2b, None), (None, None)):
        got, _, _ = sd.check_segments(target, before, after, flow, lab, b2, a2, origin=cases.ORIGIN, label="a d2 missing")
        assert np.array_equal(got["table"][:, 3:13:2], full["table"][:, 3:13:2]) and (b2 is not None or not got["table"][:, 4:13:2].any())
        assert a2 is not None or not got["table"][:, 15:24:2].any()
    sd.check_segments(target, before, after, None, lab, d2b, d2a, origin=cases.ORIGIN, label="no flow")
    sd.check_segments(target, before, None, flow, lab, d2b, d2a, origin=cases.ORIGIN, same_after=True, label="after is before")


def test_reruns_and_streams_give_identical_bits():
    target, before, after, flow, lab, d2b, d2a = _scene((2500, 3000, 500), 4000, 81)
    first, _, image = sd.check_segments(target, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, label="first")
    built = sd.build(target, cases.ORIGIN)
    runs, images = [sd.segments(image, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN, ws_poison=p) for p in (0x00, 0xA5)], []
    for s in (torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)):
        with torch.cuda.stream(s):
            images.append(sd.build(target, cases.ORIGIN, poison=0x11))
            runs.append(sd.segments(image, before, after, flow, lab, d2b, d2a, origin=cases.ORIGIN))
    for other in runs:
        for k in ("table", "code_before", "code_after", "info"):
            assert other[k].tobytes() == first[k].tobytes(), k
    assert all(i["image"].tobytes() == built["image"].tobytes() == image.tobytes() and i["info"].tolist() == built["info"].tolist() for i in images)


# ---- the verdict ------------------------------------------------------------------------------------------------------------
def test_four_spoiled_segments_each_get_their_verdict():
    from icp_flow_amd import utils_eval
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)   # noqa: E731
    src, flow, labels, dst = cases.verdict()
    ps, pf, pl, pd = up(src), up(flow), up(labels), up(dst)
    table, num, info, d2b, d2a = utils_eval.segment_residual_device(ps, ps, pf, pl, pd, radius=2.0, per_row=True)
    report = utils_eval.segment_residual_read(table, num, info, 2.0)
    image = utils_eval.sight_image(pd)
    assert image.image.shape == (2, 64, 1024) and image.info.tolist()[0] == 0 and image.params.as_dict() == S.START
    seen = utils_eval.segment_sight(image, ps, ps, pf, pl, d2b, d2a)
    worst = seen.annotate(report.worst())
    assert {e["label"]: e["verdict"] for e in worst} == {cases.PULLED: "seen through", cases.WALLED: "lost from view",
                                                         cases.FLUNG: "lost from view", cases.UNSEEN: "lost from view"}
    assert all(e["far_rows"] == 220 for e in worst) and seen.labels.tolist() == report.labels.tolist() and seen.rows.tolist() == report.rows.tolist()
    assert sum(seen.info[k] for k in utils_eval.SIGHT_INFO_NAMES[6:]) == len(src) and seen.info["after_bad_rows"] == 0
    lines = utils_eval.format_segment_sight(worst)
    assert len(lines) == 4 and all(line.startswith("residual segment: ") and line.endswith(e["verdict"]) for line, e in zip(lines, worst))
    # the rows' own codes, and the nearest range on request
    codes, near = utils_eval.line_of_sight(image, ps, pf, near=True)
    v = S.view((0, 0, 0))
    want_image, _ = S.build(v, dst)
    want_code, want_near, want_counts = S.query(v, want_image, src, flow)
    assert np.array_equal(codes.cpu().numpy(), want_code) and np.array_equal(near.cpu().numpy().view(np.uint32), want_near.view(np.uint32))
    assert image.last_counts.tolist() == want_counts and np.array_equal(image.image.cpu().numpy().view(np.uint32), want_image)
    assert utils_eval.line_of_sight(image, ps).dtype == torch.int32
    _, _, _, cb, ca = utils_eval.segment_sight_device(image, ps, ps, pf, pl, d2b, d2a, Lmax=64, per_row=True)
    assert torch.equal(ca, codes) and torch.equal(cb, utils_eval.line_of_sight(image, ps))
    with pytest.raises(ValueError, match="distinct labels"):
        utils_eval.segment_sight(image, ps, ps, pf, pl, Lmax=7)
    # another origin and a coarser image are parameters of the call
    other = utils_eval.sight_image(pd, origin=(0.0, 0.0, 1.5), W=512, H=32)
    assert other.image.shape == (2, 32, 512) and other.params.W == 512 and other.origin.tolist() == [0.0, 0.0, 1.5]


# ---- end to end -------------------------------------------------------------------------------------------------------------
LOST = 1.0      # the object the destination frame does not see: its segment stays where the ego pose left it


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    from icp_flow_amd import frame_pairs
    root = tmp_path_factory.mktemp("sight")
    for seed in (41, 42, 43):
        d = rcases.rigid_pair(seed)
        seen = d["labels_src"] != LOST
        fp = frame_pairs.FramePair(d["points_src"], d["points_dst"][seen], d["labels_src"], d["labels_src"][seen], d["pose"], name=f"rigid_{seed}")
        frame_pairs.save_frame_pair(str(root / f"fp_{seed}.npz"), fp)
    return str(root)


def test_run_stream_with_the_attribute(directory):
    from icp_flow_amd import frame_pairs, utils_eval
    paths = frame_pairs.list_frame_pairs(directory)
    a = frame_pairs.default_args(max_points=2048)
    a.residual, a.residual_segments = 2.0, True
    plain = frame_pairs.run_stream(a, paths, DEV)
    assert "residual_sight" not in plain and "ms_sight_per_frame_pair" not in plain
    added = ("seen_through", "excused", "far_rows", "verdict")
    assert not any(k in e for e in plain["residual_segments"]["worst"] for k in added)
    blocks = {}
    for origin, in_flight in ((True, 1), (True, 4), ((0.0, 0.0, 1.5), 1)):
        a.residual_sight = origin
        s = frame_pairs.run_stream(a, paths, DEV, in_flight=in_flight)
        assert [k for k in s if k not in plain] == ["residual_sight", "ms_sight_per_frame_pair"] and s["ms_sight_per_frame_pair"] > 0
        assert json.dumps(s["residual"], sort_keys=True) == json.dumps(plain["residual"], sort_keys=True)
        core = [{k: v for k, v in e.items() if k not in added} for e in s["residual_segments"]["worst"]]
        assert json.dumps(core, sort_keys=True) == json.dumps(plain["residual_segments"]["worst"], sort_keys=True)
        assert {k: v for k, v in s["residual_segments"].items() if k != "worst"} == {k: v for k, v in plain["residual_segments"].items() if k != "worst"}
        for e in s["residual_segments"]["worst"]:
            assert list(e)[-4:] == list(added) and e["verdict"] in utils_eval.SIGHT_VERDICTS and 0 <= e["seen_through"] + e["excused"] <= e["far_rows"] <= e["rows"]
        blocks[(origin, in_flight)] = json.dumps(s["residual_sight"], sort_keys=True)
    assert blocks[(True, 1)] == blocks[(True, 4)]
    block = json.loads(blocks[(True, 1)])
    assert sorted(block) == ["far", "origin", "params", "verdicts"] and block["origin"] == [0.0, 0.0, 0.0] and block["far"] == 0.1
    assert block["params"] == S.START and sorted(block["verdicts"]) == sorted(utils_eval.SIGHT_VERDICTS)
    assert sum(block["verdicts"].values()) == plain["residual_segments"]["segments_listed"]
    assert json.loads(blocks[((0.0, 0.0, 1.5), 1)])["origin"] == [0.0, 0.0, 1.5]


def test_the_command_line_prints_the_verdicts(directory, capsys):
    from icp_flow_amd import frame_pairs
    frame_pairs.main([directory, "--max-points", "2048", "--residual", "--residual-segments", "--residual-sight", "0", "0", "1.5"])
    text = capsys.readouterr().out
    summary = json.loads(text.strip().splitlines()[-1])
    assert summary["residual_sight"]["origin"] == [0.0, 0.0, 1.5] and summary["ms_sight_per_frame_pair"] > 0
    lines = [line for line in text.splitlines() if line.startswith("residual segment: frame pair:")]
    assert len(lines) == len(summary["residual_segments"]["worst"]) >= 3 and all("far rows:" in line for line in lines)

"""GPU: the trust byte (icpflow_flow_trust, csrc/trust.hip) against its numpy restatement (tests/trust_restatement.py),
array_equal throughout: the tables and the per-row arrays are made in numpy (tests/trust_cases.py), so that every threshold is
hit exactly; every call runs on guarded, poisoned outputs (tests/trust_device.py).  Then the chain end to end: frame_trust on a
small frame pair, run_sequences with save_trust, run_stream with residual_trust.  The restatement itself is held against the
host logic it restates on the CPU (tests/test_trust.py)."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trust_cases as cases                   # noqa: E402
import trust_device as td                     # noqa: E402
import trust_restatement as T                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = td.DEV
F = np.float32


def _case(L, n, seed, P=30, stride=10, sight=True, codes=True, flow=True, **table):
    labels = cases.labels_for(L, seed)
    resid, seen, what = cases.tables(labels, seed + 1, **table)
    r = cases.rows(n, labels, seed + 2, codes=codes and sight, flow=flow)
    return dict(after=r["after"], flow=r["flow"], labels=r["labels"], d2=r["d2"], code=r["code"], resid=resid, sight=seen if sight else None,
                pairs=cases.pair_rows(P, stride, labels, seed + 3), table_labels=labels, what=what)


@pytest.mark.parametrize("n", [0, 1, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 70001])
def test_row_counts_over_the_thread_and_the_workgroup(n):
    """the edges of a four-row thread and of a 1024-row workgroup; exactly d_trust[0, n) is written (the guards)"""
    c = _case(40, n, 100 + n)
    got, _ = td.check(c, label=f"n {n}")
    assert len(got["trust"]) == n and got["counts"][:8].sum() + got["counts"][15] == n
    if n == 0:
        assert got["counts"].tolist() == [0] * 16 and len(got["segment"]) == 40


@pytest.mark.parametrize("full", [False, True], ids=["Lmax=L", "Lmax=4096"])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 1024, 1025, 4096])
def test_segment_counts(L, full):
    """one thread per segment over the edges of a wave and of a workgroup, the keys of up to 4096 segments in LDS; d_segment
    from *d_num on stays as it was"""
    c = _case(L, 3000, 300 + L)
    got, _ = td.check(c, label=f"L {L}", Lmax=4096 if full else L)
    assert len(got["segment"]) == L and got["counts"][15] > 0


@pytest.mark.parametrize("stride", [1, 10])
@pytest.mark.parametrize("P", [0, 1, 1023, 1024, 1025, 5000])
def test_pair_counts_over_the_tiles(P, stride):
    """the pair labels through LDS in tiles of 1024; a label listed twice counts once"""
    c = _case(300, 2000, 500 + P, P=P, stride=stride)
    if P >= 2:
        col = c["pairs"][:, 0]
        assert col[0].view(np.uint32) == col[P - 1].view(np.uint32) and T.key(col[:1])[0] in T.key(c["table_labels"])     # listed twice
    got, _ = td.check(c, label=f"P {P} stride {stride}")
    matched = (got["segment"] & T.MATCHED) != 0
    assert matched.any() == (P > 0) and (P < 1000 or 50 < matched.sum() < 250)


def test_every_class_is_counted():
    c = _case(200, 20000, 700)
    got, exp = td.check(c, label="classes")
    counts = got["counts"]
    want_rows = (exp["trust"][exp["has_segment"]] & T.ROW_MASK)
    assert all((want_rows == k).any() for k in range(7)) and all((((exp["segment"] >> 3) & 3) == k).any() for k in range(4))   # on the input
    assert (counts[:7] > 0).all() and counts[7] == 0 and (counts[8:12] > 0).all() and (counts[12:] > 0).all()
    assert counts[:8].sum() == 20000 - counts[15] and counts[14] == ((got["trust"] & T.KEEP) != 0).sum()
    # ROW 7: far rows without a code
    bare = dict(c, sight=None, code=None)
    got7, _ = td.check(bare, label="classes, no codes")
    assert got7["counts"][7] == counts[2:7].sum() and got7["counts"][2:7].tolist() == [0] * 5 and got7["counts"][0] == counts[0]
    assert got7["counts"][:8].sum() == 20000 - got7["counts"][15] and got7["counts"][14] == ((got7["trust"] & T.KEEP) != 0).sum()


def test_the_thresholds_hit_exactly():
    """a mean equal to `above` is not listed and the next double is; seen == share * far is not "seen through"; no good row;
    no far row; d2 == far2 is NEAR and the float above it is not"""
    labels = np.array([1, 2, 3, 4, 5, 6], F)
    parts = [cases.tables(labels[k: k + 1], 9, mean=m, far=f) for k, (m, f) in
             enumerate((("equal", "all seen"), ("just above", "all seen"), ("above", "tie"), ("above", "no far row"), ("no good row", "all seen"),
                        ("above", "lost from view")))]
    resid, sight = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert resid[0, 16] / resid[0, 10] == 0.1 and resid[1, 16] / resid[1, 10] == np.nextafter(0.1, 1)
    assert sight[2, 19] == 0.5 * sight[2, 15:24:2].sum() > 0 and sight[3, 15:24:2].sum() == 0 and resid[4, 10] == 0
    far2 = F(0.1) * F(0.1)
    n = 6 * 3
    c = dict(after=np.ones((n, 3), F), flow=None, labels=np.repeat(labels, 3), d2=np.tile(np.array([far2, np.nextafter(far2, F(1)), 0.0], F), 6),
             code=np.full(n, 3, np.int32), resid=resid, sight=sight, pairs=None)
    got, _ = td.check(c, label="thresholds")
    assert ((got["segment"] >> 3) & 3).tolist() == [0, 1, 3, 3, 0, 2]
    assert (got["trust"] & 7).tolist() == [1, 3, 1] * 6
    assert ((got["trust"] & T.KEEP) != 0).tolist() == [True] * 3 + [False] * 9 + [True] * 6
    # the same tables with share 0.4: the tie is a majority now; far = 0: only d2 == 0 is near
    got, _ = td.check(c, label="share 0.4", params=dict(share=0.4))
    assert ((got["segment"] >> 3) & 3).tolist() == [0, 1, 1, 3, 0, 2]
    got, _ = td.check(c, label="far 0", params=dict(far=0.0))
    assert (got["trust"] & 7).tolist() == [3, 3, 1] * 6


def test_labels_zeros_nans_absent_and_skipped():
    """-0.0 and +0.0 are one segment; a NaN label has a segment of its own and its signalling form finds it; a label no segment
    has gives byte 0; both skip labels are SKIPPED with FIT 0 whatever their mean"""
    labels = cases.labels_for(8, 5)
    assert np.isnan(labels).sum() == 2 and {-1e8, -1.0, 0.0} <= set(labels[~np.isnan(labels)].tolist()) and 9.5 not in labels
    resid, sight, _ = cases.tables(labels, 6, mean="far above", far="all seen")
    rows = np.concatenate([labels, np.array([-0.0, 9.5, -np.inf], F), np.array([cases.SNAN, 0x7FC12346, 0xFF812345], np.uint32).view(F)])
    n = len(rows)
    pairs = np.zeros((3, 10), F)
    pairs[:, 0] = (-0.0, np.nan, -1.0)
    c = dict(after=np.ones((n, 3), F), flow=None, labels=rows, d2=np.zeros(n, F), code=np.full(n, 3, np.int32), resid=resid, sight=sight, pairs=pairs)
    got, exp = td.check(c, label="labels")
    at = {int(b): k for k, b in enumerate(labels.view(np.uint32).tolist())}
    t = got["trust"]
    assert t[8] == t[at[0]] != 0 and (t[at[0]] & T.MATCHED)                              # -0.0 finds 0.0's segment, matched by the pair row -0.0
    assert t[11] == t[at[int(cases.QNAN)]] != 0 and not (t[11] & T.MATCHED)              # the signalling NaN finds its quiet form; NaN == NaN fails
    assert t[9] == 0 and t[10] == 0 and t[12] == 0 and t[13] == 0                        # absent: 9.5, -inf, another payload, another sign
    assert got["counts"][15] == 4 and exp["has_segment"].sum() == n - 4
    for skip in (-1e8, -1.0):
        b = t[at[int(F(skip).view(np.uint32))]]
        assert b & T.SKIPPED and (b >> 3) & 3 == 0 and b & T.KEEP
    assert (t[at[int(F(-1.0).view(np.uint32))]] & T.MATCHED) and got["counts"][13] == 2
    listed = [k for k in range(8) if labels[k] not in (F(-1e8), F(-1.0))]
    assert all((t[k] >> 3) & 3 == 1 and not t[k] & T.KEEP for k in listed)


@pytest.mark.parametrize("num", [0, -1, -5000])
def test_no_segments_or_an_overflow_reported(num):
    c = _case(40, 2500, 900)
    got, _ = td.check(c, label=f"num {num}", num=num, Lmax=64)
    assert not got["trust"].any() and got["counts"].tolist() == [0] * 15 + [2500] and len(got["segment"]) == 0


def test_without_a_sight_table():
    c = _case(150, 5000, 1000, sight=False)
    got, _ = td.check(c, label="no sight")
    rows = got["trust"] & 7
    assert set(rows.tolist()) == {0, 1, 7} and set(((got["segment"] >> 3) & 3).tolist()) == {0, 3}
    assert not (got["trust"][((got["trust"] >> 3) & 3) == 3] & T.KEEP).any()


def test_bad_rows_and_no_flow():
    """a bad row (inf, NaN, 2e6; by the point or by the flow alone) has ROW 0, keeps its segment's bits and is not kept"""
    c = _case(60, 6000, 1100)
    got, exp = td.check(c, label="bad rows")
    bad = ~T.good_rows(c["after"], c["flow"]) & exp["has_segment"]
    by_flow = bad & T.good_rows(c["after"], None)
    assert bad.sum() > 100 and by_flow.sum() > 40
    t = got["trust"][bad]
    assert ((t & 7) == 0).all() and not (t & T.KEEP).any() and (t & 0x78).any() and got["counts"][0] == bad.sum()
    seg = exp["segment"][np.searchsorted(T.key(c["table_labels"]), T.key(c["labels"][bad]))]
    assert np.array_equal(t & 0x78, seg)
    none, _ = td.check(dict(c, flow=None), label="no flow")
    assert none["counts"][0] == (~T.good_rows(c["after"], None) & exp["has_segment"]).sum() < got["counts"][0]


def test_two_runs_and_a_second_stream_leave_the_same_bits():
    c = _case(500, 50000, 1200, P=2000)
    first = td.run(c)
    again = td.run(c)
    side = torch.cuda.Stream(device=DEV)
    other = td.run(c, stream=side)
    for got in (again, other):
        assert all(first[k].tobytes() == got[k].tobytes() for k in ("trust", "segment", "counts"))


def test_a_refused_call_writes_nothing():
    c = _case(40, 1000, 1300)
    E_ARG, E_LIMIT = -1, -3
    td.run(c, Lmax=4097, expect=E_LIMIT, expect_message="at most 4096 segments")
    td.run(c, spoil=dict(Lmax=0), expect=E_ARG, expect_message="Lmax must be at least 1")
    td.run(c, spoil=dict(n=-1), expect=E_ARG, expect_message="a negative size")
    td.run(c, spoil=dict(stride=0), expect=E_ARG, expect_message="pair_stride")
    td.run(c, spoil=dict(pairs=None), expect=E_ARG, expect_message="no pair rows")
    td.run(c, spoil=dict(code=None), expect=E_ARG, expect_message="a sight table without")
    td.run(c, spoil=dict(sight=None), expect=E_ARG, expect_message="codes without a sight table")
    for name in ("after", "labels", "resid", "num", "d2"):
        td.run(c, spoil={name: None}, expect=E_ARG, expect_message="null pointer")
    for over in (dict(above=-1.0), dict(far=float("nan")), dict(far=2e3), dict(share=1.0)):
        td.run(c, params=over, expect=E_ARG, expect_message="must lie in")
    from icp_flow_amd import _lib
    p = _lib.TrustParams.defaults()
    p.struct_size = 48
    td.run(c, params=p, expect=E_ARG, expect_message="struct_size = 48")
    td.check(c, label="after the refusals")


# ---- the Python layer and the chain -----------------------------------------------------------------------------------------
def _registered(d):
    """the crafted frame pair as a registration would hand it over"""
    from icp_flow_amd import frame_pairs
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"])
    out = dict(flow=torch.from_numpy(d["flow"]).to(DEV), pairs=torch.from_numpy(d["pairs"]).to(DEV), labels_src=torch.from_numpy(d["labels_src"]).to(DEV))
    return fp, out


def test_a_small_frame_pair_end_to_end():
    """frame_trust with an origin: the bytes equal the restatement applied to the tables and per-row arrays read back from the
    same three calls; the cluster flowed into free space is "seen through" and none of its rows is kept, the occluded one is
    "lost from view" and kept"""
    from icp_flow_amd import frame_pairs, utils_eval
    d = cases.frame_pair()
    fp, out = _registered(d)
    trust, counts = frame_pairs.frame_trust(fp, out, DEV, 2.0, origin=(0.0, 0.0, 0.0))
    assert trust.dtype == torch.uint8 and trust.is_cuda and tuple(trust.shape) == (len(d["points_src"]),)
    ps, pd, flow, lab = (torch.from_numpy(d[k]).to(DEV) for k in ("points_src", "points_dst", "flow", "labels_src"))
    table, num, _, d2b, d2a = utils_eval.segment_residual_device(ps, ps, flow, lab, pd, 2.0, per_row=True)
    image = utils_eval.sight_image(pd, (0.0, 0.0, 0.0))
    seen, _, _, _, code = utils_eval.segment_sight_device(image, ps, ps, flow, lab, d2b, d2a, far=0.1, per_row=True)
    L = int(num.item())
    assert L == 8
    exp = T.trust(d["points_src"], d["flow"], d["labels_src"], table.cpu().numpy(), seen.cpu().numpy(), L, d2a.cpu().numpy(), code.cpu().numpy(),
                  d["pairs"][:, 0])
    t = trust.cpu().numpy()
    assert np.array_equal(t, exp["trust"]) and np.array_equal(counts.words(), exp["counts"])
    labels = d["labels_src"]
    fit = {float(v): int((exp["segment"][c] >> 3) & 3) for c, v in enumerate(table[:L, 0].cpu().tolist())}
    assert fit[cases.MISFLOWED] == 1 and fit[cases.OCCLUDED] == 2 and sum(fit.values()) == 3
    assert not (t[labels == cases.MISFLOWED] & T.KEEP).any() and ((t[labels == cases.MISFLOWED] >> 3) & 3 == 1).all()
    assert ((t[labels == cases.OCCLUDED] >> 3) & 3 == 2).all() and (t[labels == cases.OCCLUDED] & T.KEEP).all()
    assert counts.kept == len(labels) - 300 and counts.kept_share() == counts.kept / len(labels) and counts.no_segment == 0
    assert torch.equal(utils_eval.trust_keep(trust), (trust & 128) != 0) and int(utils_eval.trust_keep(trust).sum()) == counts.kept
    # without an origin: the residual alone, a listed segment is undecided and dropped; flow_trust is the same call with its read-back
    bare, bare_counts = frame_pairs.frame_trust(fp, out, DEV, 2.0)
    b = bare.cpu().numpy()
    assert set((b & 7).tolist()) == {1, 7} and ((b[np.isin(labels, (cases.MISFLOWED, cases.OCCLUDED))] >> 3) & 3 == 3).all()
    assert bare_counts.kept == len(labels) - 600 and bare_counts.fit.tolist() == [1200, 0, 0, 600]
    again, again_counts = utils_eval.flow_trust(ps, flow, lab, table, num, d2a, out["pairs"], seen, code)
    assert torch.equal(again, trust) and np.array_equal(again_counts.words(), counts.words())
    with pytest.raises(ValueError, match="come together"):
        utils_eval.flow_trust_device(ps, flow, lab, table, num, d2a, out["pairs"], seen, None)


@pytest.fixture(scope="module")
def sequence(tmp_path_factory):
    """one synthetic F = 3 sequence file and the arguments of its run"""
    from icp_flow_amd import frame_pairs, synthetic
    tmp = tmp_path_factory.mktemp("trust")
    d = synthetic.make_sequence(seed=3, num_frames=3, n_objects=6, n_max=400)
    sd = (d["nonground"] & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    os.makedirs(os.path.join(tmp, "val"))
    path = os.path.join(tmp, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=d["nonground"].astype(np.int64))
    a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
    a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.05, False, "ego_motion_gt"
    return dict(path=path, args=a)


def _spied(monkeypatch):
    """frame_trust as the drivers call it, its results kept: [(gap, bytes uint8 [Ns], counts int64 [16], origin)]"""
    from icp_flow_amd import frame_pairs, pair_judges
    real, calls = frame_pairs.frame_trust, []

    def spy(fp, out, device, radius, origin=None, params=None):
        trust, counts = real(fp, out, device, radius, origin, params)
        calls.append((fp.gap, trust.cpu().numpy().copy(), counts.words(), origin, radius))
        return trust, counts

    monkeypatch.setattr(frame_pairs, "frame_trust", spy)           # where run_sequences reads it
    monkeypatch.setattr(pair_judges, "frame_trust", spy)           # where run_stream's TrustJudge reads it
    return calls


def _meters(metrics):
    return {name: [getattr(m, f + "_data") for f in ("epe", "accs", "accr", "outlier", "Routlier")] + [m.num_data if hasattr(m, "num_data") else None]
            for name, m in metrics.items()}


def test_run_sequences_saves_the_bytes_beside_the_flow(sequence, monkeypatch):
    from icp_flow_amd import frame_pairs, utils_eval
    path, a = sequence["path"], SimpleNamespace(**vars(sequence["args"]))
    a.save_flows = True
    saved = frame_pairs.flow_file(path, False)
    plain = frame_pairs.run_sequences(a, [path], DEV)
    with np.load(saved) as z:
        assert sorted(z.files) == ["ego_motion", "scene_flow"]                       # without the flag: today's file
        flow_bytes = z["scene_flow"].tobytes()
    assert "trust" not in plain and "ms_trust_per_sequence" not in plain
    t = frame_pairs.load_sequence_sample(path, a)["time_indice"]
    for origin in (True, (0.0, 0.0, 1.5)):
        calls = _spied(monkeypatch)
        a.save_trust = origin
        res = frame_pairs.run_sequences(a, [path], DEV)
        assert [k for k in res if k not in plain] == ["trust", "ms_trust_per_sequence"] and res["ms_trust_per_sequence"] > 0
        assert {k: v for k, v in res.items() if k in plain and not k.startswith("ms_") and k != "metrics"} == \
               {k: v for k, v in plain.items() if not k.startswith("ms_") and k != "metrics"}
        assert json.dumps(_meters(res["metrics"]), sort_keys=True, default=repr) == json.dumps(_meters(plain["metrics"]), sort_keys=True, default=repr)
        assert sorted(c[0] for c in calls) == [1, 2] and all(c[3] == (None if origin is True else origin) and c[4] == 2.0 for c in calls)
        want = np.zeros(len(t), np.uint8)
        for gap, bytes_, _, _, _ in calls:
            want[np.flatnonzero(t == gap)] = bytes_
        with np.load(saved, allow_pickle=False) as z:
            assert sorted(z.files) == ["ego_motion", "scene_flow", "trust", "trust_params"]
            got, params = z["trust"], json.loads(str(z["trust_params"]))
            assert z["scene_flow"].tobytes() == flow_bytes
        assert got.dtype == np.uint8 and np.array_equal(got, want) and not got[t == 0].any() and got[t != 0].any()
        total = utils_eval.TrustCounts()
        for c in calls:
            total.add(utils_eval.TrustCounts(c[2]))
        assert res["trust"] == dict(total.summary(), params=params) and total.n() == int((t != 0).sum())
        assert params["radius"] == 2.0 and params["origin"] == (None if origin is True else list(origin)) and ("sight" in params) == (origin is not True)
        assert total.rows[2:7].sum() == (0 if origin is True else total.rows[2:7].sum()) and (origin is not True or total.rows[7] > 0)
        monkeypatch.undo()


def test_run_stream_counts_are_the_sum_over_its_frame_pairs(sequence, monkeypatch):
    from icp_flow_amd import frame_pairs, utils_eval
    path, a = sequence["path"], SimpleNamespace(**vars(sequence["args"]))
    a.residual, a.residual_segments = 2.0, True
    plain = frame_pairs.run_stream(a, [path], DEV)
    assert "residual_trust" not in plain
    for sight in (None, (0.0, 0.0, 1.5)):
        calls = _spied(monkeypatch)
        a.residual_trust = True
        if sight is not None:
            a.residual_sight = sight
        s = frame_pairs.run_stream(a, [path], DEV)
        extra = [k for k in s if k not in plain]
        assert extra == (["residual_trust"] if sight is None else ["residual_sight", "ms_sight_per_frame_pair", "residual_trust"])
        assert json.dumps(s["residual"], sort_keys=True) == json.dumps(plain["residual"], sort_keys=True)
        assert len(calls) == s["frame_pairs"] == 2 and all(c[3] == sight and c[4] == 2.0 for c in calls)
        total = utils_eval.TrustCounts()
        for c in calls:
            total.add(utils_eval.TrustCounts(c[2]))
        block = s["residual_trust"]
        assert {k: block[k] for k in total.summary()} == total.summary() and block["kept_share"] == total.kept / total.n()
        assert block["line_of_sight"] == (sight is not None) and block["ms_trust_per_frame_pair"] > 0
        assert block["rows_evaluated"] == s["evaluated_points"] and block["epe_kept"] >= 0 and block["epe_dropped"] >= 0
        assert json.loads(json.dumps(s))["residual_trust"]["kept"] == total.kept
        monkeypatch.undo()

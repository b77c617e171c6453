"""CPU-only: the trust byte (icpflow_flow_trust, csrc/trust.hip; utils_eval.flow_trust, frame_pairs.frame_trust, run_stream's
`--residual-trust`, run_sequences' `--save-trust`) as far as it goes without a GPU -- the exports, every refusal with its code and
message (all of them come before any launch), the command line, the restatement the GPU tests compare against
(tests/trust_restatement.py) held against the host logic it restates (SegmentResidual.worst, SegmentSight.annotate) on random
tables with the thresholds hit exactly, the conditions the GPU tests' frame pair must meet, and the saved file's keys."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_residual_restatement as sr     # noqa: E402
import sight_restatement as S                 # noqa: E402
import trust_cases as cases                   # noqa: E402
import trust_restatement as T                 # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_LIMIT = -1, -3
F = np.float32
NAMES = ("icpflow_flow_trust_default_params", "icpflow_flow_trust")
ONE = ctypes.c_void_p(4096)


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib, build, utils_eval
    assert _lib.VERSION == 215
    for name, n_args in zip(NAMES, (1, 18)):
        assert hasattr(_lib._L, name) and len(_lib.SIGNATURES[name][1]) == n_args and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert "trust.hip" in build.SOURCES and "trust.hpp" in build.HEADERS and "labelkey.hpp" in build.HEADERS
    hdr = open(os.path.join(REPO, "include", "icpflow_hip.h")).read()
    assert "#define ICPFLOW_TRUST_COUNTS 16" in hdr and all(name + "(" in hdr for name in NAMES) and "} icpflow_trust_params_t;" in hdr
    assert (_lib.TRUST_COUNTS, _lib.TRUST_MAX_SEGMENTS) == (16, 4096)
    # size_t, three doubles, two floats on LP64
    assert ctypes.sizeof(_lib.TrustParams) == 40 and [k for k, _ in _lib.TrustParams._fields_] == ["struct_size", "above", "far", "share", "skip"]
    p = _lib.TrustParams.defaults()
    assert p.struct_size == 40 and p.as_dict() == dict(above=0.1, far=0.1, share=0.5, skip=[-1e8, -1.0])
    assert p.above == utils_eval.RESIDUAL_EDGES[1] and tuple(p.skip) == tuple(F(s) for s in utils_eval.RESIDUAL_SKIP_LABELS)
    assert _lib.TrustParams.defaults(share=0.25, skip=(3.0, 4.0)).as_dict() == dict(above=0.1, far=0.1, share=0.25, skip=[3.0, 4.0])
    with pytest.raises(TypeError, match="no parameter"):
        _lib.TrustParams.defaults(radius=2.0)
    # the bits, in Python and in the restatement
    assert (utils_eval.TRUST_ROW_MASK, utils_eval.TRUST_FIT_SHIFT, utils_eval.TRUST_FIT_MASK) == (T.ROW_MASK, T.FIT_SHIFT, T.FIT_MASK) == (7, 3, 3)
    assert (utils_eval.TRUST_MATCHED, utils_eval.TRUST_SKIPPED, utils_eval.TRUST_KEEP) == (T.MATCHED, T.SKIPPED, T.KEEP) == (32, 64, 128)
    assert len(utils_eval.TRUST_ROW_NAMES) == 8 and len(utils_eval.TRUST_FIT_NAMES) == 4
    # the shared key lives in one place
    table_hip = open(os.path.join(REPO, "icp_flow_amd", "csrc", "table.hip")).read()
    assert '#include "labelkey.hpp"' in table_hip and "uint32_t label_key(" not in table_hip and "uint32_t sortable(" not in table_hip


def _trust(**over):
    """the call with arguments that pass every check: each test below spoils one (nothing is launched by a refused call)"""
    from icp_flow_amd import _lib
    a = dict(after=ONE, flow=None, labels=ONE, n=10, resid=ONE, sight=None, num=ONE, Lmax=64, d2=ONE, code=None, pairs=ONE, P=4, stride=10,
             params={}, trust=ONE, segment=ONE, counts=ONE)
    a.update(over)
    p = a["params"] if a["params"] is None or isinstance(a["params"], _lib.TrustParams) else _lib.TrustParams.defaults(**a["params"])
    rc = _lib._L.icpflow_flow_trust(a["after"], a["flow"], a["labels"], a["n"], a["resid"], a["sight"], a["num"], a["Lmax"], a["d2"], a["code"],
                                    a["pairs"], a["P"], a["stride"], None if p is None else ctypes.byref(p), a["trust"], a["segment"], a["counts"], None)
    return rc, _lib._L.icpflow_last_error().decode()


def test_every_refusal_has_its_code_and_message():
    from icp_flow_amd import _lib
    fn = "icpflow_flow_trust"
    for name in ("after", "labels", "resid", "num", "d2", "params", "trust", "segment", "counts"):
        rc, msg = _trust(**{name: None})
        assert rc == E_ARG and fn + ": null pointer" in msg, name
    for over in (dict(n=-1), dict(P=-1), dict(n=-5, P=-5)):
        rc, msg = _trust(**over)
        assert rc == E_ARG and "a negative size" in msg and fn in msg, over
    rc, msg = _trust(n=(1 << 29) + 1)
    assert rc == E_LIMIT and "rows a cloud" in msg and fn in msg
    for Lmax in (0, -1):
        rc, msg = _trust(Lmax=Lmax)
        assert rc == E_ARG and "Lmax must be at least 1" in msg, Lmax
    for Lmax in (4097, 1 << 20):
        rc, msg = _trust(Lmax=Lmax)
        assert rc == E_LIMIT and "at most 4096 segments" in msg, Lmax
    for stride in (0, -10):
        rc, msg = _trust(stride=stride)
        assert rc == E_ARG and "pair_stride must be at least 1" in msg, stride
    rc, msg = _trust(pairs=None)
    assert rc == E_ARG and "P = 4 and no pair rows" in msg
    rc, msg = _trust(sight=ONE)
    assert rc == E_ARG and "a sight table without line-of-sight codes" in msg
    rc, msg = _trust(code=ONE)
    assert rc == E_ARG and "line-of-sight codes without a sight table" in msg
    rc, msg = _trust(code=ONE, n=0, after=None, labels=None, d2=None, trust=None)
    assert rc == E_ARG and "line-of-sight codes without a sight table" in msg
    p = _lib.TrustParams.defaults()
    p.struct_size = 32
    rc, msg = _trust(params=p)
    assert rc == E_ARG and "struct_size = 32" in msg and "40 bytes" in msg
    for name in ("above", "far"):
        for value in (-0.01, 1000.5, float("nan"), float("inf"), -float("inf")):
            rc, msg = _trust(params={name: value})
            assert rc == E_ARG and f"{name} must lie in [0, 1e3]" in msg, (name, value)
    for value in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        rc, msg = _trust(params=dict(share=value))
        assert rc == E_ARG and "share must lie in [0, 1)" in msg, value
    assert _lib._L.icpflow_flow_trust_default_params(None) == E_ARG and "null pointer" in _lib._L.icpflow_last_error().decode()


def test_there_is_no_cpu_path():
    from icp_flow_amd import frame_pairs, utils_eval
    x, lab, d2 = torch.zeros(8, 3), torch.zeros(8), torch.zeros(8)
    table, num = torch.zeros((4, 18), dtype=torch.float64), torch.ones(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.flow_trust_device(x, None, lab, table, num, d2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.flow_trust(x, x, lab, table, num, d2, torch.zeros((2, 10)), torch.zeros((4, 24), dtype=torch.float64), torch.zeros(8, dtype=torch.int32))
    fp = frame_pairs.FramePair(x.numpy(), x.numpy(), lab.numpy(), lab.numpy())
    with pytest.raises(RuntimeError, match="no CPU path"):
        frame_pairs.frame_trust(fp, dict(flow=x, pairs=torch.zeros((0, 10))), "cpu", 2.0)
    assert utils_eval.trust_keep(torch.tensor([0, 1, 128, 255, 127], dtype=torch.uint8)).tolist() == [False, False, True, True, False]
    assert utils_eval.trust_keep(np.array([129, 2], np.uint8)).tolist() == [True, False]


def test_the_counts_add_and_summarise():
    from icp_flow_amd import utils_eval
    a, b = utils_eval.TrustCounts(np.arange(16)), utils_eval.TrustCounts()
    assert b.n() == 0 and np.isnan(b.kept_share()) and b.words().tolist() == [0] * 16
    assert a.words().tolist() == list(range(16)) and a.n() == 28 + 15 and a.kept_share() == 14 / 43
    assert b.add(a) is b and b.add(a).words().tolist() == [2 * k for k in range(16)] and b.kept_share() == a.kept_share()
    s = a.summary()
    assert list(s) == ["n", "rows", "fit", "matched", "skipped", "kept", "no_segment", "kept_share"] and json.loads(json.dumps(s)) == s
    assert s["rows"]["seen_through"] == 2 and s["fit"]["lost_from_view"] == 10 and s["no_segment"] == 15


def _stub_register(args, fp, device):
    return dict(pairs=torch.zeros((2, 10)), transformations=torch.eye(4).repeat(2, 1, 1), flow=torch.from_numpy(fp.gt_flow.copy()))


def test_the_flags_parse_and_their_combinations_are_checked():
    from icp_flow_amd import frame_pairs, synthetic
    before = dict(frame_pairs.DEFAULT_ARGS)
    ap = frame_pairs.argument_parser()
    ns = ap.parse_args(["dir"])
    assert ns.residual_trust is False and ns.save_trust is None
    assert ap.parse_args(["dir", "--residual", "--residual-segments", "--residual-trust"]).residual_trust is True
    assert ap.parse_args(["dir", "--protocol", "reference", "--save-flows", "--save-trust"]).save_trust == []
    assert ap.parse_args(["dir", "--protocol", "reference", "--save-flows", "--save-trust", "0", "-0.5", "1.7"]).save_trust == [0.0, -0.5, 1.7]
    for argv in (["dir", "--residual-trust"], ["dir", "--residual", "--residual-trust"], ["dir", "--residual", "0.5", "--residual-trust"]):
        with pytest.raises(SystemExit, match="--residual-trust goes with --residual --residual-segments"):
            frame_pairs.main(argv)
    for argv in (["dir", "--save-trust"], ["dir", "--protocol", "reference", "--save-trust", "0", "0", "1"]):
        with pytest.raises(SystemExit, match="--save-trust goes with --save-flows"):
            frame_pairs.main(argv)
    with pytest.raises(SystemExit, match="the origin's three"):
        frame_pairs.main(["dir", "--protocol", "reference", "--save-flows", "--save-trust", "1", "2"])
    assert frame_pairs.DEFAULT_ARGS == before
    for name in ("residual_trust", "save_trust"):
        assert name not in frame_pairs.DEFAULT_ARGS and not hasattr(frame_pairs.default_args(), name)
    # the drivers' own checks, and without the attribute the summary of today
    d = synthetic.make_frame_pair(seed=1, n_objects=3, n_max=60, n_background=50)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    a = frame_pairs.default_args()
    keys = list(frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register))
    a.residual_trust = False
    assert list(frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)) == keys and "residual_trust" not in keys
    a.residual_trust = True
    with pytest.raises(ValueError, match="needs args.residual and args.residual_segments"):
        frame_pairs.run_stream(a, [fp], "cpu", register_fn=_stub_register)
    a.num_frames, a.save_trust = 2, True
    with pytest.raises(ValueError, match="save_trust needs args.save_flows"):
        frame_pairs.run_sequences(a, [], "cpu")
    a.save_flows, a.save_trust = True, (0.0, 1.0)
    with pytest.raises(ValueError, match="an origin"):
        frame_pairs.run_sequences(a, [], "cpu")


# ---- the restatement against the host logic it restates -------------------------------------------------------------------------
def _host_verdicts(resid, sight, pairs, above, share, skip):
    """SegmentResidual.worst then SegmentSight.annotate -> {label: (verdict, matched)} of the listed segments"""
    from icp_flow_amd import utils_eval
    worst = utils_eval.SegmentResidual.from_table(resid, utils_eval.RESIDUAL_EDGES, 2.0).worst(pairs=pairs, above=above, skip=skip)
    if sight is not None:
        utils_eval.SegmentSight.from_table(sight).annotate(worst, share=share)
    return {e["label"]: (e.get("verdict", "undecided"), e["matched"]) for e in worst}


def test_the_restated_segment_bits_are_the_host_logic_on_random_tables():
    """320 table pairs of 12 segments (NaN labels left out: annotate cannot look a NaN label up, a dict key), with the pair rows
    beside them; the equalities the header decides are asserted as conditions on the inputs"""
    seen = dict(equal=0, tie=0, no_good=0, no_far=0, skip=set(), zero_matched=0, listed=0, verdicts=set(), matched_listed=0, tables=0)
    for seed in range(320):
        labels = cases.labels_for(14, 1000 + seed)
        labels = labels[~np.isnan(labels)]
        resid, sight, what = cases.tables(labels, 2000 + seed)
        pairs = cases.pair_rows(6, 2 + seed % 3, labels, 3000 + seed)
        above, share = ((0.1, 0.5), (0.1, 0.5), (0.05, 0.4), (0.25, 0.6))[seed % 4]
        skip = (-1e8, -1.0) if seed % 5 else (7.0, float(labels[-1]))
        for with_sight in (False, True):
            seg = T.segment_bytes(resid, sight if with_sight else None, pairs[:, 0], above, share, skip)
            host = _host_verdicts(resid, sight if with_sight else None, pairs, above, share, skip)
            fit = (seg >> T.FIT_SHIFT) & T.FIT_MASK
            listed = {float(labels[c]): (T.FIT_NAMES[fit[c]], bool(seg[c] & T.MATCHED)) for c in range(len(labels)) if fit[c]}
            assert listed == host, (seed, with_sight)
            if not with_sight:
                assert set(fit.tolist()) <= {0, 3}
            seen["tables"] += 1
        skipped = (seg & T.SKIPPED) != 0
        assert skipped.sum() == (2 if seed % 5 else int(7.0 in labels) + 1) and (fit[skipped] == 0).all()
        mean = np.divide(resid[:, 16], resid[:, 10], out=np.full(len(labels), np.nan), where=resid[:, 10] != 0)
        far = sight[:, 15:24:2].sum(axis=1)
        for c in range(len(labels)):
            if mean[c] == above:                                   # a mean exactly equal to `above`: not listed
                assert fit[c] == 0 and what[c][0] == "equal"
                seen["equal"] += 1
            if fit[c] and sight[c, 19] == share * far[c]:          # seen exactly share * far: not "seen through"
                assert fit[c] != 1
                seen["tie"] += 1 if far[c] else 0
                seen["no_far"] += 0 if far[c] else 1               # no far row: 0 > 0 fails twice, undecided
                assert far[c] or fit[c] == 3
            if resid[c, 10] == 0:                                  # a segment without a good row: no mean, not listed
                assert fit[c] == 0
                seen["no_good"] += 1
            if skipped[c] and mean[c] > above:                     # a skip label that fits badly is still not listed
                seen["skip"].add(float(labels[c]))
            if labels[c] == 0.0 and seg[c] & T.MATCHED:
                assert (pairs[:, 0] == 0.0).any() and np.signbit(pairs[pairs[:, 0] == 0.0, 0]).all()   # -0.0 in the pair rows
                seen["zero_matched"] += 1
        seen["listed"] += int((fit != 0).sum())
        seen["verdicts"] |= set(fit.tolist())
        seen["matched_listed"] += int(((fit != 0) & ((seg & T.MATCHED) != 0)).sum())
    assert seen["tables"] == 640 and seen["equal"] >= 20 and seen["tie"] >= 20 and seen["no_good"] >= 20 and seen["no_far"] >= 20
    assert {-1e8, -1.0} <= seen["skip"] and seen["zero_matched"] >= 10 and seen["listed"] >= 500 and seen["verdicts"] == {0, 1, 2, 3}
    assert seen["matched_listed"] >= 100


def test_the_means_around_the_threshold_divide_as_stated():
    """the "equal" segment's mean IS the double 0.1 and the "just above" one's is the next double: the listing turns on `>`"""
    by = {m[0]: m for m in cases.MEANS}
    assert by["equal"][2] / by["equal"][1] == 0.1 and by["just above"][2] / by["just above"][1] == np.nextafter(0.1, 1)
    labels = np.array([3.0, 4.0], F)
    for mean, fit in (("equal", 0), ("just above", 1), ("no good row", 0), ("far above", 1)):
        resid, sight, _ = cases.tables(labels, 5, mean=mean, far="seen through")
        assert ((T.segment_bytes(resid, sight, []) >> 3) & 3).tolist() == [fit, fit], mean
    for far, fit in (("seen through", 1), ("lost from view", 2), ("tie", 3), ("no far row", 3), ("at first return", 3), ("excused tie", 3), ("all seen", 1),
                     ("all behind", 2)):
        resid, sight, _ = cases.tables(labels, 6, mean="above", far=far)
        assert ((T.segment_bytes(resid, sight, []) >> 3) & 3).tolist() == [fit, fit], far
        assert ((T.segment_bytes(resid, None, []) >> 3) & 3).tolist() == [3, 3]


def test_the_restated_rows_find_their_segments_by_the_tables_key():
    labels = cases.labels_for(40, 7)
    resid, sight, _ = cases.tables(labels, 8)
    r = cases.rows(3000, labels, 9)
    seg = T.segment_bytes(resid, sight, cases.pair_rows(30, 10, labels, 10)[:, 0])
    t, has = T.row_bytes(r["after"], r["flow"], r["labels"], resid, len(labels), seg, r["d2"], r["code"])
    bits = r["labels"].view(np.uint32)
    at = {float(v): c for c, v in enumerate(labels.tolist()) if v == v}
    zero, snan, qnan = np.flatnonzero(bits == 0x80000000), np.flatnonzero(bits == cases.SNAN), np.flatnonzero(bits == cases.QNAN)
    assert len(zero) > 5 and len(snan) > 5 and len(qnan) > 5
    assert has[zero].all() and has[snan].all() and has[qnan].all()
    c0, cn = at[0.0], int(np.flatnonzero(labels.view(np.uint32) == cases.QNAN)[0])
    assert ((t[zero] & 0x78) == seg[c0]).all() and ((t[snan] & 0x78) == seg[cn]).all() and ((t[qnan] & 0x78) == seg[cn]).all()
    absent = ~np.isin(T.key(r["labels"]), T.key(labels))
    assert absent.sum() > 50 and not has[absent].any() and (t[absent] == 0).all() and has[~absent].all()
    good = T.good_rows(r["after"], r["flow"])
    assert (~good).sum() > 50 and ((t[~good] & T.ROW_MASK) == 0).all() and ((t[~good] & T.KEEP) == 0).all()
    assert ((t[~good & has] & 0x78) == seg[np.searchsorted(T.key(labels), T.key(r["labels"][~good & has]))]).all()   # a bad row keeps its segment's bits
    far2 = F(0.1) * F(0.1)
    on = has & good & (r["d2"] == far2)
    assert on.sum() > 100 and ((t[on] & T.ROW_MASK) == T.ROW_NEAR).all()                       # d2 == far2 is NEAR
    over = has & good & (r["d2"] == np.nextafter(far2, F(1)))
    assert over.sum() > 100 and ((t[over] & T.ROW_MASK) >= 2).all()
    c = T.counts(t, has)
    assert c[:8].sum() == 3000 - c[15] and c[15] == absent.sum() and c[14] == ((t & T.KEEP) != 0).sum() and (c[:7] > 0).all() and (c[8:12] > 0).all()
    # without codes no row is 2 .. 6 and the far ones are 7; *d_num <= 0: every byte 0
    t2, has2 = T.row_bytes(r["after"], r["flow"], r["labels"], resid, len(labels), seg, r["d2"], None)
    assert set((t2 & T.ROW_MASK).tolist()) == {0, 1, 7} and T.counts(t2, has2)[7] == c[2:7].sum() and c[7] == 0
    for num in (0, -41):
        t0, has0 = T.row_bytes(r["after"], r["flow"], r["labels"], resid, num, seg, r["d2"], r["code"])
        assert not t0.any() and not has0.any() and T.counts(t0, has0).tolist() == [0] * 15 + [3000]


def test_the_frame_pair_spoils_two_segments_each_in_its_own_way():
    """the scene of the GPU's end-to-end test, on the restatements of the three calls it chains"""
    from icp_flow_amd import utils_eval
    d = cases.frame_pair()
    src, flow, labels, dst = d["points_src"], d["flow"], d["labels_src"], d["points_dst"]
    assert 2900 <= len(src) <= 3100 and len(np.unique(labels)) == 8
    res = sr.residual(src, src, flow, labels, dst, 2.0, utils_eval.RESIDUAL_EDGES)
    resid = sr.table18(res)
    v = S.view((0, 0, 0))
    image, _ = S.build(v, dst)
    seen = S.segments(v, image, src, src, flow, labels, res["d2_before"], res["d2_after"], far=0.1)
    got = T.trust(src, flow, labels, resid, seen["table"], len(resid), res["d2_after"], seen["code_after"], d["pairs"][:, 0])
    fit = {float(resid[c, 0]): int((got["segment"][c] >> 3) & 3) for c in range(len(resid))}
    assert fit == {-1e8: 0, -1.0: 0, 0.0: 0, cases.MISFLOWED: 1, 2.0: 0, 3.0: 0, cases.OCCLUDED: 2, 5.0: 0}
    t = got["trust"]
    assert got["has_segment"].all() and not (t[labels == cases.MISFLOWED] & T.KEEP).any() and ((t[labels == cases.MISFLOWED] & 7) == 2).sum() > 250
    occluded = t[labels == cases.OCCLUDED]
    assert ((occluded & 7) == 4).sum() > 250 and (occluded & T.KEEP).all()                       # behind the wall: excused, kept
    for k in (0.0, 2.0, 3.0, 5.0):
        assert (t[labels == k] == (T.KEEP | T.MATCHED | T.ROW_NEAR)).all(), k
    assert (t[labels == -1.0] & T.SKIPPED).all() and (t[labels == -1e8] & T.SKIPPED).all() and not (t[labels < 0] & T.MATCHED).any()
    assert got["counts"][14] == len(src) - 300 and got["counts"][12] == 1800 and got["counts"][13] == 1200


# ---- the saved file -------------------------------------------------------------------------------------------------------------
def test_the_saved_file_gains_two_keys_only_with_the_bytes(tmp_path):
    from icp_flow_amd import frame_pairs
    pts = np.zeros((4, 3), F)
    fps = [frame_pairs.FramePair(pts, pts, pose=np.eye(4), gap=1, pose_source="ego_motion_gt")]
    flow = torch.arange(30, dtype=torch.float32).reshape(10, 3)
    path = str(tmp_path / "val" / "seq.npz")
    out = frame_pairs.save_sequence_flow(path, flow, fps, 2)
    with np.load(out) as z:
        assert sorted(z.files) == ["ego_motion", "scene_flow"]
        flow_bytes, pose_bytes = z["scene_flow"].tobytes(), z["ego_motion"].tobytes()
    trust = torch.tensor([0, 0, 0, 0, 129, 161, 2, 90, 7, 255], dtype=torch.uint8)
    params = dict(radius=2.0, origin=[0.0, 0.0, 1.5], above=0.1, far=0.1, share=0.5, skip=[-1e8, -1.0])
    assert frame_pairs.save_sequence_flow(path, flow, fps, 2, trust=trust, trust_params=params) == out
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == ["ego_motion", "scene_flow", "trust", "trust_params"]
        assert z["trust"].dtype == np.uint8 and z["trust"].tolist() == trust.tolist()
        assert z["scene_flow"].dtype == np.float64 and z["ego_motion"].dtype == np.float64 and z["ego_motion"].shape == (2, 4, 4)
        assert z["scene_flow"].tobytes() == flow_bytes and z["ego_motion"].tobytes() == pose_bytes
        assert json.loads(str(z["trust_params"])) == params
    for bad in (trust[:9], trust.to(torch.int32)):
        with pytest.raises(ValueError, match="rows of uint8"):
            frame_pairs.save_sequence_flow(path, flow, fps, 2, trust=bad)

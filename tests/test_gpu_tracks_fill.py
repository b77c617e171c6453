"""GPU: the track fill against its numpy restatement (tests/fill_restatement.py) -- icpflow_object_tracks_missing and
icpflow_pairs_fill_candidates word for word, on poisoned, guarded outputs (tests/fill_device.py) -- and run_stream --tracks
--tracks-fill end to end on a synthetic sample with a hook that deletes one pair row of one gap before the tracks: a track at
constant velocity gets its pair back, the box that truly left its line does not, and a sample with every pair in place is left
as it is."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as fc                       # noqa: E402
import fill_restatement as fr                 # noqa: E402
import repair_cases as rc                     # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def dv():
    from icp_flow_amd import _lib
    assert all(hasattr(_lib._L, name) for name in ("icpflow_object_tracks_missing", "icpflow_pairs_fill_candidates"))
    import fill_device
    return fill_device


# --------------------------------------------------------------------------------------------------------------------- the plan

def _check(dv, case, label=""):
    return dv.check_missing(case["obs"], case["T"], case["segments"], case["num"], case["gaps"], case["seconds"], label=label)


@pytest.mark.parametrize("M", (0, 1, 255, 256, 257, 1025))
def test_the_plan_equals_the_restatement_at_every_number_of_observations(dv, M):
    _, counts, _ = _check(dv, fc.plan_at(M, 3, (40, 7, 64), 64, 100 + M), f"M = {M}")
    assert M < 255 or (counts.sum(axis=0) > 0).all()


@pytest.mark.parametrize("G, num, Lmax", ((1, (0,), 64), (1, (1,), 1), (3, (63, 64, 65), 65), (3, (64, -3, 2), 64), (64, tuple(range(64)), 64), (2, (4096, 300), 4096)))
def test_the_plan_at_every_number_of_slots_and_segments(dv, G, num, Lmax):
    case = fc.plan_at(300, G, num, Lmax, 7 * G + Lmax)
    plan, counts, _ = _check(dv, case, f"G = {G}, num = {num}")
    assert all(counts[g].sum() == 0 for g in range(G) if num[g] <= 0)


def test_the_plan_on_the_hand_made_tables_and_on_300_seeded_ones(dv):
    for rows, gaps in ((fc.on_a_line(seen=(1, 3)), (1, 2, 3)), (fc.on_a_line(seen=(1,)), (1, 2, 3)), (fc.on_a_line(seen=(1,)) * 2, (1, 2, 3)),
                       (fc.on_a_line(seen=(1, 2, 3)), (1, 2, 3)), (fc.on_a_line(seen=(1, 2, 2, 3)), (2,)), (fc.on_a_line(seen=(1, 3), off={3: (0.0, 1.0, 0.0)}), (1, 2, 3))):
        seg, num, h_gap, h_sec = fc.slots(gaps)
        dv.check_missing(rows, 1, seg, num, h_gap, h_sec)
    seg, num, h_gap, h_sec = fc.slots((1, 2, 3))
    for y, missing in ((0.25, 1.0), (float(np.nextafter(0.25, 1.0)), 0.0)):          # inner = m2 exactly, and the next double above
        plan, _, _ = dv.check_missing([fc.obs(0, 1, 0.5, (0.0, y, 0.0)), fc.obs(0, 3, 0.5, (0.0, -y, 0.0))], 1, seg, num, h_gap, h_sec, max_residual=0.25)
        assert plan[1, 1, 0] == missing
    seen = np.zeros(4, np.int64)
    for k, case in enumerate(fc.random_plans(300)):
        seen += _check(dv, case, f"table {k}")[1].sum(axis=0)
    assert (seen > 0).all()


def test_the_plan_is_bit_identical_on_a_rerun_and_on_a_second_stream(dv):
    case = fc.plan_at(700, 3, (64, 64, 30), 64, 5)
    args = (case["obs"], case["T"], case["segments"], case["num"], case["gaps"], case["seconds"])
    first = dv.run_missing(*args)[3]
    assert dv.run_missing(*args)[3] == first and dv.run_missing(*args, stream=torch.cuda.Stream())[3] == first


def test_the_suspects_are_bit_for_bit_what_they_were_on_their_own_tables(dv):
    """the walk of icpflow_object_tracks_suspects moved into the device function the plan above shares: its restatement, which did
    not move, still holds word for word on the repair's own hand-made and seeded tables"""
    import repair_device
    for rows in (rc.one_outlier(bad=2), rc.one_outlier(gaps=(1, 2), bad=2), rc.one_outlier(gaps=(1, 2), bad=0) + [rc.obs(0, 2, 0.25, (0.5, -0.25, 0.0625))]):
        repair_device.check_plan(rows, 1)
    seen = np.zeros(4, np.int64)
    for k, (obs, T) in enumerate(rc.random_tables(300)):
        seen += repair_device.check_plan(obs, T, label=f"table {k}")[1]
    assert (seen > 0).all()


# -------------------------------------------------------------------------------------------------------------- the candidates

@pytest.mark.parametrize("K", (0, 1, 63, 64, 65, 257))
def test_the_candidates_equal_the_restatement_at_every_number_of_rows(dv, K):
    case = fc.random_candidates(K, 300, 100, 40 + K)
    choice, counts, raw = dv.check_candidates(case["q"], case["boxes"], case["num"], case["pairs"], label=f"K = {K}")
    assert counts[:3].sum() == K and (K < 3 or counts[2] >= 2)                         # three rows aimed at one segment: two lose it
    assert dv.run_candidates(case["q"], case["boxes"], case["num"], case["pairs"], stream=torch.cuda.Stream())[2] == raw


@pytest.mark.parametrize("num, P", ((0, 0), (1, 1), (255, 1023), (256, 1024), (257, 1025), (1025, 100), (4096, 2500)))
def test_the_candidates_at_every_number_of_segments_and_pair_rows(dv, num, P):
    case = fc.random_candidates(9, num, P, num + P, Lmax=max(num, 1) if num != 1025 else 2000)
    _, counts, raw = dv.check_candidates(case["q"], case["boxes"], case["num"], case["pairs"], label=f"num = {num}, P = {P}")
    assert counts[:3].sum() == 9 and (num < 255 or counts[0] > 0)
    assert dv.run_candidates(case["q"], case["boxes"], case["num"], case["pairs"])[2] == raw          # a rerun is bit-identical


def test_the_candidates_on_the_hand_made_tables(dv):
    boxes = fc.box_table([fc.box(4.0, (3.0, 4.0, 1.0))])
    assert dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 1, np.zeros((0, 10)), radius=5.0)[0][0, 4] == 5.0          # d2 = radius^2 exactly
    assert dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 1, np.zeros((0, 10)), radius=float(np.nextafter(5.0, 0.0)))[0][0, 0] == 1.0
    boxes = fc.box_table([fc.box(1.0, (0.5, 0.0, 0.0)), fc.box(2.0, (-0.5, 0.0, 0.0)), fc.box(3.0, (0.0, 0.5, 0.0)), fc.box(7.0, (10.0, 10.0, 0.0))])
    assert dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 4, np.zeros((0, 10)))[0][0, 1] == 0.0                       # a tie: the lower c
    choice, counts, _ = dv.check_candidates([[10.25, 10.0, 0.0], [10.0, 10.125, 0.0], [10.0, 9.875, 5.0], [0.5, 0.25, 0.0]], boxes, 4, np.zeros((0, 10)))
    assert choice[:, 0].tolist() == [2, 0, 2, 0] and counts.tolist() == [2, 0, 2, 4]                                 # a tie: the lower k
    boxes = fc.box_table([fc.box(1.0, (0.0, 0.0, 0.0)), fc.box(2.0, (0.1, 0.0, 0.0), rows=10001), fc.box(3.0, (0.2, 0.0, 0.0), k=-1),
                          fc.box(4.0, (0.3, 0.0, 0.0), rows=10000), fc.box(5.0, (0.9, 0.0, 0.0))])
    assert dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 5, fc.pair_rows([1.0, 9.0]))[0][0, :3].tolist() == [0, 3, 4.0]
    dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 3, fc.pair_rows([1.0], stride=1))
    for labels, matched in (((-0.0, np.nan), [0.0]), ((0.0, np.nan), [-0.0, np.nan]), ((16777217.0, 2.0), [16777216.0])):
        boxes = fc.box_table([fc.box(labels[0], (0.0, 0.0, 0.0)), fc.box(labels[1], (0.5, 0.0, 0.0))])
        assert dv.check_candidates([[0.0, 0.0, 0.0]], boxes, 2, fc.pair_rows(matched))[0][0, 1] == 1.0               # +-0 one label, a NaN equals none
    boxes = fc.box_table([fc.box(1.0, (np.nan, 0.0, 0.0)), fc.box(2.0, (0.0, np.nan, 0.0)), fc.box(3.0, (0.75, 0.0, np.nan))])
    choice, _, _ = dv.check_candidates([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], boxes, 3, np.zeros((0, 10)))
    assert choice[:, 0].tolist() == [0, 1] and choice[0, 1] == 2.0


def test_the_device_wrappers_give_what_the_raw_calls_give(dv):
    from icp_flow_amd import utils_tracks
    case = fc.plan_at(300, 3, (64, 20, 0), 64, 9)
    plan, counts = utils_tracks.missing_device(torch.from_numpy(case["obs"]).cuda(), case["T"], torch.from_numpy(case["segments"]).cuda(),
                                               torch.from_numpy(case["num"]).cuda(), case["gaps"], case["seconds"])
    want, written, want_counts = fr.missing(case["obs"], case["T"], case["segments"], case["num"], case["gaps"], case["seconds"])
    want[~written] = 0.0                                      # the wrapper's plan is allocated as zeros
    dv.same(plan.cpu().numpy().reshape(-1, 14), want.reshape(-1, 14), "missing_device")
    assert counts.cpu().tolist() == want_counts.tolist()
    case = fc.random_candidates(20, 300, 100, 3)
    choice, counts = utils_tracks.fill_candidates_device(torch.from_numpy(case["q"]).cuda(), torch.from_numpy(case["boxes"]).cuda(),
                                                         torch.tensor([case["num"]], dtype=torch.int32).cuda(), torch.from_numpy(case["pairs"]).cuda())
    want, want_counts = fr.candidates(case["q"], case["boxes"], case["num"], case["pairs"][:, 0])
    dv.same(choice.cpu().numpy(), want, "fill_candidates_device")
    assert counts.cpu().tolist() == want_counts.tolist()


# ------------------------------------------------------------------------------------------------------------------ end to end

def dev():
    return torch.device("cuda:0")


def _snapshot(outs):
    return [{k: out[k].detach().clone() for k in ("pairs", "transformations", "flow")} for out in outs]


def _flow(fp, out):
    from icp_flow_amd import utils_flow
    T = out["transformations"]
    src = torch.from_numpy(fp.points_src_raw if fp.points_src_raw is not None else fp.points_src).to(T.device)
    return utils_flow.flow_estimation_torch(None, src, None, out["labels_src"], None, out["pairs"], T, torch.from_numpy(fp.pose).to(T.device))


def _pair_of(out, k, j):
    """the pair row of gap j whose translation lies nearest the true displacement of object k"""
    T = out["transformations"]
    return int(torch.argmin(torch.linalg.norm(T[:, :3, 3].double().cpu() - torch.from_numpy(rc.displacement(k, j)), dim=1)))


def _run(root, name, path, delete=None, fault=False, fill=True, repair=False, **kw):
    """run_stream --cluster dbscan --tracks FILE [--tracks-fill] [--tracks-repair] --objects FILE over the sample, with a hook of
    the test's own around frame_tracks and one around the objects' accounting: the pair row of `delete` = (object, frame) is
    deleted and that gap's flow recomputed on the device as the gap is delivered (before its objects and the tracks see it); the
    hook around frame_tracks writes the repair test's fault, keeps every gap's tensors before and after, and lists the library
    calls made in between"""
    from icp_flow_amd import _lib, frame_pairs, pair_judges
    real, real_call, real_account, kept = pair_judges.frame_tracks, _lib.call, pair_judges.ObjectJudge.account, dict(calls=[])

    def counted(fn, *a):
        kept["calls"].append(fn)
        return real_call(fn, *a)

    def account(self, number, fp, out):
        # the deletion, once, before the gap's objects are accounted: the objects' lines and the tracks see the same pair rows
        if delete is not None and fp.gap == delete[1] and "pair" not in kept:
            p = _pair_of(out, *delete)
            keep = [k_ for k_ in range(len(out["pairs"])) if k_ != p]
            kept["pair"], kept["deleted_labels"], kept["undeleted"] = p, out["pairs"][p, :2].tolist(), out["transformations"][p].clone()
            out["pairs"], out["transformations"] = out["pairs"][keep].clone(), out["transformations"][keep].clone()
            out["flow"] = _flow(fp, out)
        return real_account(self, number, fp, out)

    def hooked(fps, outs, *a, **k):
        if fault:
            g = rc.FAULTED_FRAME - 1
            T = outs[g]["transformations"].clone()
            p = _pair_of(outs[g], rc.FAULTED, rc.FAULTED_FRAME)
            shift = torch.eye(4, dtype=T.dtype, device=T.device)
            shift[:3, 3] = torch.from_numpy(rc.FAULT).to(T)
            T[p] = shift @ T[p]
            outs[g]["transformations"] = T
            outs[g]["flow"] = _flow(fps[g], outs[g])
        kept["fps"], kept["before"] = fps, _snapshot(outs)
        _lib.call = counted
        try:
            seen = real(fps, outs, *a, **k)
        finally:
            _lib.call = real_call
        kept["after"], kept["outs"] = _snapshot(outs), outs
        return seen

    a = frame_pairs.default_args(**fc.CLUSTER)
    a.tracks, a.objects, a.sweep_seconds = str(root / f"tracks_{name}.jsonl"), str(root / f"objects_{name}.jsonl"), fc.SWEEP_SECONDS
    if fill:
        a.tracks_fill = True
    if repair:
        a.tracks_repair = True
    pair_judges.frame_tracks, pair_judges.ObjectJudge.account = hooked, account
    try:
        summary = frame_pairs.run_stream(a, [path], dev(), **kw)
    finally:
        pair_judges.frame_tracks, pair_judges.ObjectJudge.account = real, real_account
    return dict(summary=summary, tracks=[json.loads(line) for line in open(a.tracks)], objects=[json.loads(line) for line in open(a.objects)], **kept)


FILLED, HONEST, OTHER = (fc.FILLED, fc.FILLED_FRAME), (fc.HONEST, fc.HONEST_FRAME), (1, 1)


@pytest.fixture(scope="module")
def end_to_end(dv, tmp_path_factory):
    root = tmp_path_factory.mktemp("fill")
    path = str(root / "sample.npz")
    np.savez(path, **fc.scene()["arrays"])
    return dict(path=path, plain=_run(root, "plain", path, fill=False), whole=_run(root, "whole", path), filled=_run(root, "filled", path, delete=FILLED),
                honest=_run(root, "honest", path, delete=HONEST), flight=_run(root, "flight", path, delete=FILLED, in_flight=4),
                repair=_run(root, "repair", path, delete=OTHER, fault=True, fill=False, repair=True),
                both=_run(root, "both", path, delete=OTHER, fault=True, repair=True))


def _same_tensors(a, b):
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t   # noqa: E731
    return all(x[k].shape == y[k].shape and torch.equal(bits(x[k]), bits(y[k])) for x, y in zip(a, b) for k in x)


def test_end_to_end_a_deleted_pair_of_a_track_at_constant_velocity_is_filled(end_to_end):
    run, plain = end_to_end["filled"], end_to_end["plain"]
    g, p = fc.FILLED_FRAME - 1, run["pair"]
    fills = run["tracks"][0]["fill"]
    print("filled run:", fills, run["summary"]["tracks_fill"])
    # exactly one fill, accepted, with the deleted labels, appended behind the gap's old rows
    assert len(fills) == 1 and fills[0]["accepted"] is True and fills[0]["reason"] == "accepted" and (fills[0]["gap"], fills[0]["frame_pair"]) == (g, g)
    assert fills[0]["labels"] == run["deleted_labels"] and fills[0]["e_new"] < fills[0]["e_old"] and fills[0]["distance"] <= 0.2
    before, after = run["before"], run["after"]
    P = len(before[g]["pairs"])
    assert fills[0]["pair"] == P and len(after[g]["pairs"]) == P + 1 and len(after[g]["transformations"]) == P + 1
    assert after[g]["pairs"][P, :2].tolist() == run["deleted_labels"]
    # the appended box-centre displacement against the synthetic truth, within max_residual (the policy's own number)
    entry = [e for e in run["objects"][g]["objects"] if e["pair"] == P][0]
    d = np.asarray(entry["velocity"]) * run["objects"][g]["seconds"]
    print("filled displacement", d, "truth", rc.displacement(*FILLED))
    assert np.linalg.norm(d[:2] - rc.displacement(*FILLED)[:2]) <= 0.2
    # printed, not asserted: how far the appended transform lies from the one the undeleted run registered for that pair
    gap = (after[g]["transformations"][P] - run["undeleted"]).abs().max().item()
    print(f"appended transform against the undeleted run's: largest entry difference {gap:.6f}")
    assert torch.equal(run["undeleted"], plain["after"][g]["transformations"][p])
    # the old rows of that gap and every tensor of the other gaps keep every bit
    assert _same_tensors([before[0], before[2]], [after[0], after[2]])
    assert torch.equal(before[g]["pairs"], after[g]["pairs"][:P]) and torch.equal(before[g]["transformations"], after[g]["transformations"][:P])
    # the flow rows of that cluster are flow_estimation_torch's on the new tensors; the other rows are unchanged
    mine = run["outs"][g]["labels_src"] == after[g]["pairs"][P, 0]
    want = _flow(run["fps"][g], dict(run["outs"][g], pairs=after[g]["pairs"], transformations=after[g]["transformations"]))
    assert int(mine.sum()) > 100 and torch.equal(after[g]["flow"][mine], want[mine]) and not torch.equal(after[g]["flow"][mine], before[g]["flow"][mine])
    assert torch.equal(after[g]["flow"][~mine], before[g]["flow"][~mine])
    # the track is observed in three gaps and consistent afterwards
    track = [t for t in run["tracks"][0]["tracks"] if t["track"] == fills[0]["track"]][0]
    assert track["gaps"] == [1, 2, 3] and track["consistent"] and track["judged"]
    block = run["summary"]["tracks_fill"]
    assert (block["missing"], block["retried"], block["accepted"]) == (1, 1, 1) and sum(block["reasons"].values()) == 1
    assert block["observed_before"] == block["observed_after"] and block["judged_before"] == block["judged_after"] and run["summary"]["ms_tracks_fill_per_sample"] > 0


def test_end_to_end_the_box_that_left_its_line_is_never_filled(end_to_end):
    run = end_to_end["honest"]
    fills = run["tracks"][0]["fill"]
    print("honest run:", fills, run["summary"]["tracks_fill"])
    assert len(fills) == 1 and fills[0]["gap"] == fc.HONEST_FRAME - 1 and fills[0]["accepted"] is False and fills[0]["pair"] is None
    assert fills[0]["reason"] in ("no_candidate", "off_prediction", "not_better")
    assert _same_tensors(run["before"], run["after"])                                  # every tensor is bit for bit the deleted state
    block = run["summary"]["tracks_fill"]
    assert (block["missing"], block["accepted"]) == (1, 0) and sum(block["reasons"].values()) == 1


def test_end_to_end_nothing_deleted_nothing_filled_nothing_launched_beyond_the_plan(end_to_end):
    run, plain = end_to_end["whole"], end_to_end["plain"]
    assert run["tracks"][0]["fill"] == [] and "fill" not in plain["tracks"][0]
    launching = lambda calls: [c for c in calls if not c.endswith(("_default_params", "_workspace_bytes"))]   # noqa: E731  (those two kinds enqueue nothing)
    assert [c for c in run["calls"] if c not in plain["calls"]] == ["icpflow_object_tracks_missing"]
    assert len(launching(run["calls"])) == len(launching(plain["calls"])) + 1 and launching(run["calls"])[: len(launching(plain["calls"]))] == launching(plain["calls"])
    assert _same_tensors(run["before"], run["after"]) and _same_tensors(run["after"], plain["after"])
    assert run["tracks"][0]["tracks"] == plain["tracks"][0]["tracks"] and run["tracks"][0]["observations"] == plain["tracks"][0]["observations"]
    assert run["objects"] == plain["objects"]
    assert [k for k in run["summary"] if k not in plain["summary"]] == ["tracks_fill", "ms_tracks_fill_per_sample"]
    timing = ("ms_per_frame_pair", "frame_pairs_per_s", "ms_objects_per_frame_pair", "ms_tracks_per_sample", "objects_file", "tracks_file")   # (and the runs' own file names)
    assert {k: v for k, v in plain["summary"].items() if k not in timing} == {k: v for k, v in run["summary"].items() if k in plain["summary"] and k not in timing}
    block = run["summary"]["tracks_fill"]
    assert (block["missing"], block["retried"], block["accepted"]) == (0, 0, 0) and not any(block["reasons"].values())


def test_end_to_end_four_in_flight_give_the_same_fill(end_to_end):
    run, flight = end_to_end["filled"], end_to_end["flight"]
    assert flight["tracks"] == run["tracks"] and flight["summary"]["tracks_fill"] == run["summary"]["tracks_fill"]
    assert _same_tensors(run["after"], flight["after"])
    assert [[(e["pair"], e["track"], e["velocity"]) for e in line["objects"]] for line in flight["objects"]] == \
        [[(e["pair"], e["track"], e["velocity"]) for e in line["objects"]] for line in run["objects"]]


def test_end_to_end_with_the_repair_the_fill_follows_it(end_to_end):
    both, alone = end_to_end["both"], end_to_end["repair"]
    print("both:", both["summary"]["tracks_repair"], both["summary"]["tracks_fill"], both["tracks"][0]["fill"])
    assert both["summary"]["tracks_repair"] == alone["summary"]["tracks_repair"] and both["tracks"][0]["repair"] == alone["tracks"][0]["repair"]
    assert both["summary"]["tracks_repair"]["accepted"] == 1
    fills = both["tracks"][0]["fill"]
    g = OTHER[1] - 1
    assert len(fills) == 1 and fills[0]["accepted"] is True and fills[0]["gap"] == g and fills[0]["labels"] == both["deleted_labels"]
    # the fill ran on the repaired tracks: what it started from is what the repair alone ended with
    block = both["summary"]["tracks_fill"]
    assert block["observed_before"] == alone["tracks"][0]["counts"]["observed"] and block["judged_before"] == alone["tracks"][0]["counts"]["judged"]
    P = len(alone["after"][g]["pairs"])
    assert _same_tensors([alone["after"][k] for k in range(3) if k != g], [both["after"][k] for k in range(3) if k != g])
    assert torch.equal(both["after"][g]["pairs"][:P], alone["after"][g]["pairs"]) and len(both["after"][g]["pairs"]) == P + 1
    assert both["tracks"][0]["counts"]["consistent"] == 4

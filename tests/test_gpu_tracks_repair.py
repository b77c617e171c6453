"""GPU: the track repair against its numpy restatement (tests/repair_restatement.py) -- icpflow_object_tracks_suspects and
icpflow_pairs_repair_select word for word, icpflow_pairs_reregister against the entry points it is made of, all on exactly sized
0xFF workspaces with poisoned, guarded outputs (tests/repair_device.py) -- and run_stream --tracks --tracks-repair end to end on
a synthetic sample: once as it is (the box that truly leaves its line is retried and REFUSED), once with a fault written into one
gap's transforms (exactly that pair is repaired)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repair_cases as rc                     # noqa: E402
import repair_restatement as rr               # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def dv():
    from icp_flow_amd import _lib
    assert all(hasattr(_lib._L, name) for name in ("icpflow_object_tracks_suspects", "icpflow_pairs_repair_select", "icpflow_pairs_reregister"))
    import repair_device
    return repair_device


# --------------------------------------------------------------------------------------------------------------------- the plan

def _table(M, seed):
    """M observations of a handful of tracks over gaps 1 .. 5, a few of them off their line"""
    rng = np.random.default_rng(seed)
    T = max(1, M // 4)
    v = rng.normal(0, 3, (T, 3))
    rows = []
    for _ in range(M):
        t, g = int(rng.integers(-1, T + 1)), int(rng.integers(1, 6))
        d = 0.1 * g * v[t % T] + rng.normal(0, 0.3, 3) * (rng.random() < 0.15)
        rows.append(rc.obs(t, g, 0.1 * g, d))
    return np.array(rows).reshape(M, 13), T


@pytest.mark.parametrize("M", (0, 1, 255, 256, 257, 1025))
def test_the_plan_equals_the_restatement_at_every_size(dv, M):
    obs, T = _table(M, 100 + M)
    plan, counts, _ = dv.check_plan(obs, T, label=f"M = {M}")
    assert counts[0] <= M and (M < 255 or counts[3] > 0)


def test_the_plan_on_the_hand_made_tables_and_on_300_seeded_ones(dv):
    for rows in (rc.one_outlier(bad=2), rc.one_outlier(gaps=(1, 2), bad=2), rc.one_outlier(gaps=(1, 2), bad=0) + [rc.obs(0, 2, 0.25, (0.5, -0.25, 0.0625))]):
        dv.check_plan(rows, 1)
    plan, _, _ = dv.check_plan([rc.obs(0, 1, 0.5, (0.0, 0.25, 0.0)), rc.obs(0, 2, 0.5, (0.0, -0.25, 0.0)), rc.obs(0, 3, 0.5, (0.25, 0.0, 0.0))], 1, max_residual=0.25)
    assert plan[2, 6] == 0.25 and plan[2, 7] == 0.25 and plan[2, 0] == 0.0        # r2 = inner = m2 exactly: agreed, not suspect
    seen = np.zeros(4, np.int64)
    for k, (obs, T) in enumerate(rc.random_tables(300)):
        seen += dv.check_plan(obs, T, label=f"table {k}")[1]
    assert (seen > 0).all()


def test_the_plan_is_bit_identical_on_a_rerun_and_on_a_second_stream(dv):
    obs, T = _table(700, 5)
    first = dv.run_plan(obs, T)[2]
    assert dv.run_plan(obs, T)[2] == first and dv.run_plan(obs, T, stream=torch.cuda.Stream())[2] == first


# ------------------------------------------------------------------------------------------------------------------- the select

def test_the_select_equals_the_restatement_on_the_threshold_tables(dv):
    rows, want = rc.threshold_rows()
    table = rc.stack(rows)
    T_out, report, counts, _ = dv.check_select(table, 7, rc.PARAMS, "thresholds")
    assert report[:, 0].tolist() == want
    for k, reason in enumerate(want):                         # T_old bit for bit on every rejection
        assert T_out[k].tobytes() == (table["T_new"] if reason == 0 else table["T_old"])[k].tobytes()
    T_out, report, counts, _ = dv.check_select(table, -1, rc.PARAMS, "abandoned")
    assert counts.tolist() == [0, 0, 0, 0, 0, len(rows), 0, 0] and T_out.tobytes() == table["T_old"].tobytes() and not report[:, 11].any()
    dv.check_select(rc.stack([rc.select_row(errors=(np.float32(0.2), 0.9), errors_old=(0.9, 0.9))]), 1, None, "the default thres_error")


@pytest.mark.parametrize("K", (1, 63, 64, 65, 257))
def test_the_select_at_every_size(dv, K):
    rows, _ = rc.threshold_rows()
    rng = np.random.default_rng(K)
    picked = [dict(rows[int(i)]) for i in rng.integers(0, len(rows), K)]
    for r in picked:
        r["T_old"] = rng.normal(size=16).astype(F)
    T_out, _, counts, raw = dv.check_select(rc.stack(picked), 3, rc.PARAMS, f"K = {K}")
    assert counts.sum() == K and dv.run_select(rc.stack(picked), 3, rc.PARAMS, stream=torch.cuda.Stream())[3] == raw
    assert dv.run_select({k: np.zeros((0, 1)) for k in dv.SELECT_INPUTS}, 3)[2].tolist() == [0] * 8          # K = 0: eight zeros


# ------------------------------------------------------------------------------------------------------------- the reregistration

@pytest.mark.parametrize("K, N", ((1, 256), (3, 600), (17, 1100)))
def test_the_reregistration_is_its_cores_called_in_order(dv, K, N):
    from icp_flow_amd import utils_icp, utils_match
    case = dv.pair_clouds(K, 40 + K, hi=N)
    rng = np.random.default_rng(K)
    # even pairs: a poor old pose and a good prediction (to be repaired); odd pairs: the true old pose and a prediction 0.5 m off (to be kept)
    pred = case["moves"] + rng.normal(0, 0.03, (K, 3)) + np.array([[0.5 * (k % 2), 0.0, 0.0] for k in range(K)])
    T_old = np.stack([rc.translation(m + (0.0 if k % 2 else rng.normal(0, 0.2, 3))) for k, m in enumerate(case["moves"])])
    got = dv.run_reregister(case, N, T_old, pred)
    w = dv.split_words(got["words"], K)
    src, dst = got["clouds"][0].contiguous(), got["clouds"][1].contiguous()
    assert int((src[:, :, 3] > 0).sum()) == len(case["src"]) and int((dst[:, :, 3] > 0).sum()) == len(case["dst"])
    # T_new: icpflow_apply_icp through the existing wrapper on the same gathered batch
    T_new, iters = utils_icp.apply_icp(dv.REG, src, dst, got["init"], return_iterations=True)
    assert T_new.cpu().numpy().tobytes() == w["T_new"].tobytes() and int(iters.item()) == w["iters"] and w["iters"] > 0
    # the two metric sets: two icpflow_match_eval calls
    for T, tail in ((T_new, ""), (got["T_old"].view(K, 4, 4), "_old")):
        ev = utils_match.match_eval(dv.REG, src, dst, T)
        for name, t in zip(("errors", "inliers", "ratios", "ious", "translations", "rotations"), ev):
            assert t.cpu().numpy().tobytes() == w[name + tail].tobytes(), (name + tail)
    # the decision: the restatement's on those numbers
    want_T, want_report, want_counts = rr.select(w["T_new"], got["T_old"].cpu().numpy(), w["iters"], w["errors"], w["ious"], w["translations"], w["rotations"],
                                                 w["errors_old"], got["centre"], got["pred"])
    assert got["T_out"].tobytes() == want_T.tobytes() and np.array_equal(got["counts"], want_counts)
    dv.same(got["report"], want_report, f"K = {K}")
    print(f"K = {K}: reasons {got['counts'].tolist()}, iterations {w['iters']}")
    assert got["counts"][:6].sum() == K and got["counts"][0] >= 1                  # some pose is repaired, and (K > 1) some kept
    assert K == 1 or got["counts"][0] < K
    assert dv.run_reregister(case, N, T_old, pred)["raw"] == got["raw"]           # a rerun is bit-identical


def test_a_reregistration_of_no_pair_works(dv):
    case = dv.pair_clouds(1, 3, hi=100)
    got = dv.run_reregister(case, 128, np.zeros((0, 16), F), np.zeros((0, 3)), K=0)
    assert got["counts"].tolist() == [0] * 8


def test_the_device_wrappers_give_what_the_raw_calls_give(dv):
    from icp_flow_amd import utils_tracks
    obs, T = _table(300, 9)
    plan, counts = utils_tracks.suspects_device(torch.from_numpy(obs).cuda(), T)
    want, want_counts = rr.plan(obs, T)
    dv.same(plan.cpu().numpy(), want, "suspects_device")
    assert counts.cpu().tolist() == want_counts.tolist()


# ------------------------------------------------------------------------------------------------------------------ end to end

def dev():
    return torch.device("cuda:0")


def _snapshot(outs):
    return [{k: out[k].detach().clone() for k in ("pairs", "transformations", "flow")} for out in outs]


def _run(root, name, path, fault=False, repair=True, **kw):
    """run_stream --cluster dbscan --tracks FILE [--tracks-repair] --objects FILE over the sample, with a hook of the test's own
    around frame_tracks: it writes the fault (on the device, before the tracks) and keeps every gap's tensors before and after"""
    from icp_flow_amd import frame_pairs, pair_judges
    real, kept = pair_judges.frame_tracks, {}

    def hooked(fps, outs, *a, **k):
        if fault:
            g = rc.FAULTED_FRAME - 1
            T = outs[g]["transformations"].clone()
            p = int(torch.argmin(torch.linalg.norm(T[:, :3, 3].double().cpu() - torch.from_numpy(rc.displacement(rc.FAULTED, rc.FAULTED_FRAME)), dim=1)))
            shift = torch.eye(4, dtype=T.dtype, device=T.device)
            shift[:3, 3] = torch.from_numpy(rc.FAULT).to(T)
            kept["unfaulted"], T[p] = T[p].clone(), shift @ T[p]
            outs[g]["transformations"] = T
            outs[g]["flow"] = pair_judges.utils_flow.flow_estimation_torch(None, torch.from_numpy(fps[g].points_src_raw if fps[g].points_src_raw is not None else fps[g].points_src).to(T.device),
                                                                           None, outs[g]["labels_src"], None, outs[g]["pairs"], T, torch.from_numpy(fps[g].pose).to(T.device))
            kept["pair"] = p
        kept["fps"], kept["before"] = fps, _snapshot(outs)
        seen = real(fps, outs, *a, **k)
        kept["after"], kept["outs"] = _snapshot(outs), outs
        return seen

    a = frame_pairs.default_args(**rc.CLUSTER)
    a.tracks, a.objects, a.sweep_seconds = str(root / f"tracks_{name}.jsonl"), str(root / f"objects_{name}.jsonl"), rc.SWEEP_SECONDS
    if repair:
        a.tracks_repair = True
    pair_judges.frame_tracks = hooked
    try:
        summary = frame_pairs.run_stream(a, [path], dev(), **kw)
    finally:
        pair_judges.frame_tracks = real
    return dict(summary=summary, tracks=[json.loads(line) for line in open(a.tracks)], objects=[json.loads(line) for line in open(a.objects)], **kept)


@pytest.fixture(scope="module")
def end_to_end(dv, tmp_path_factory):
    root = tmp_path_factory.mktemp("repair")
    path = str(root / "sample.npz")
    np.savez(path, **rc.scene()["arrays"])
    return dict(path=path, plain=_run(root, "plain", path, repair=False), honest=_run(root, "honest", path), faulted=_run(root, "faulted", path, fault=True),
                flight=_run(root, "flight", path, fault=True, in_flight=4))


def _same_tensors(a, b):
    return all(torch.equal(x[k].view(torch.int32) if x[k].dtype == torch.float32 else x[k], y[k].view(torch.int32) if y[k].dtype == torch.float32 else y[k])
               for x, y in zip(a, b) for k in x)


def test_end_to_end_the_box_that_left_its_line_is_retried_and_refused(end_to_end):
    run, plain = end_to_end["honest"], end_to_end["plain"]
    retried = run["tracks"][0]["repair"]
    print("honest run:", retried, run["summary"]["tracks_repair"])
    assert len(retried) == 1 and retried[0]["gap"] == rc.HONEST_FRAME - 1 and retried[0]["frame_pair"] == rc.HONEST_FRAME - 1
    assert retried[0]["reason"] in ("off_prediction", "not_better") and retried[0]["accepted"] is False
    p = retried[0]["pair"]
    d = run["before"][2]["transformations"][p, :3, 3].cpu().numpy()
    assert np.linalg.norm(d[:2] - rc.displacement(rc.HONEST, rc.HONEST_FRAME)[:2]) < 0.1     # the retried pair is the honest box's
    # its transform is kept bit for bit, and no tensor of any gap differs from before the repair or from the run without the flag
    assert _same_tensors(run["before"], run["after"]) and _same_tensors(run["after"], plain["after"])
    block = run["summary"]["tracks_repair"]
    assert (block["suspects"], block["retried"], block["accepted"], block["consistent_before"], block["consistent_after"]) == (1, 1, 0, 4, 4)
    assert sum(block["reasons"].values()) == 1 and run["summary"]["ms_tracks_repair_per_sample"] > 0
    assert run["tracks"][0]["tracks"] == plain["tracks"][0]["tracks"] and run["objects"] == plain["objects"]


def test_end_to_end_without_the_flag_the_summary_has_none_of_the_new_keys(end_to_end):
    run, plain = end_to_end["honest"], end_to_end["plain"]
    assert [k for k in run["summary"] if k not in plain["summary"]] == ["tracks_repair", "ms_tracks_repair_per_sample"]
    assert "repair" not in plain["tracks"][0] and "repair" in run["tracks"][0]
    timing = ("ms_per_frame_pair", "frame_pairs_per_s", "ms_objects_per_frame_pair", "ms_tracks_per_sample", "objects_file", "tracks_file")   # (and the runs' own file names)
    assert {k: v for k, v in plain["summary"].items() if k not in timing} == {k: v for k, v in run["summary"].items() if k in plain["summary"] and k not in timing}


def test_end_to_end_a_fault_written_into_one_gap_is_repaired(end_to_end):
    from icp_flow_amd import utils_flow
    run, plain = end_to_end["faulted"], end_to_end["plain"]
    g, p = rc.FAULTED_FRAME - 1, run["pair"]
    retried = run["tracks"][0]["repair"]
    print("faulted run:", retried, run["summary"]["tracks_repair"])
    # exactly that (gap, pair) is accepted; the other suspect is the honest box's gap, refused as before
    assert [(e["gap"], e["pair"]) for e in retried if e["accepted"]] == [(g, p)] and len(retried) == 2
    assert [e["reason"] for e in retried if not e["accepted"]] == [end_to_end["honest"]["tracks"][0]["repair"][0]["reason"]]
    fixed = [e for e in retried if e["accepted"]][0]
    assert fixed["e_new"] < fixed["e_old"] and fixed["distance"] <= 0.2
    # the repaired box-centre displacement against the synthetic truth, within max_residual (the policy's own number)
    entry = [e for e in run["objects"][g]["objects"] if e["pair"] == p][0]
    d = np.asarray(entry["velocity"]) * run["objects"][g]["seconds"]
    print("repaired displacement", d, "truth", rc.displacement(rc.FAULTED, rc.FAULTED_FRAME))
    assert np.linalg.norm(d[:2] - rc.displacement(rc.FAULTED, rc.FAULTED_FRAME)[:2]) <= 0.2
    block = run["summary"]["tracks_repair"]
    assert (block["suspects"], block["retried"], block["accepted"], block["consistent_before"], block["consistent_after"]) == (2, 2, 1, 3, 4)
    track = [t for t in run["tracks"][0]["tracks"] if t["track"] == fixed["track"]][0]
    assert track["consistent"] and run["tracks"][0]["counts"]["consistent"] == 4
    # the other gaps keep every bit; in the repaired gap only that pair's transform, metric columns and flow rows change
    before, after = run["before"], run["after"]
    assert _same_tensors([before[0], before[2]], [after[0], after[2]])
    others = [k for k in range(len(after[g]["pairs"])) if k != p]
    assert torch.equal(before[g]["transformations"][others], after[g]["transformations"][others]) and torch.equal(before[g]["pairs"][others], after[g]["pairs"][others])
    assert torch.equal(before[g]["pairs"][p, :2], after[g]["pairs"][p, :2]) and not torch.equal(before[g]["pairs"][p, 2:], after[g]["pairs"][p, 2:])
    mine = run["outs"][g]["labels_src"] == after[g]["pairs"][p, 0]
    fp = run["fps"][g]
    src = torch.from_numpy(fp.points_src_raw if fp.points_src_raw is not None else fp.points_src).to(dev())
    want = utils_flow.flow_estimation_torch(None, src, None, run["outs"][g]["labels_src"], None, after[g]["pairs"], after[g]["transformations"],
                                            torch.from_numpy(fp.pose).to(dev()))
    assert int(mine.sum()) > 100 and torch.equal(after[g]["flow"][mine], want[mine]) and not torch.equal(after[g]["flow"][mine], before[g]["flow"][mine])
    assert torch.equal(after[g]["flow"][~mine], before[g]["flow"][~mine])
    # printed, not asserted: how far the repaired transform lies from the one the unfaulted run registered for that pair
    gap = (after[g]["transformations"][p] - run["unfaulted"]).abs().max().item()
    print(f"repaired transform against the unfaulted run's: largest entry difference {gap:.6f}, translation "
          f"{torch.linalg.norm(after[g]['transformations'][p][:3, 3] - run['unfaulted'][:3, 3]).item():.6f} m")
    assert torch.equal(run["unfaulted"], plain["after"][g]["transformations"][p])


def test_end_to_end_four_in_flight_give_the_same_repair(end_to_end):
    run, flight = end_to_end["faulted"], end_to_end["flight"]
    assert flight["tracks"] == run["tracks"] and flight["summary"]["tracks_repair"] == run["summary"]["tracks_repair"]
    assert _same_tensors(run["after"], flight["after"])
    assert [[(e["pair"], e["track"], e["velocity"]) for e in line["objects"]] for line in flight["objects"]] == \
        [[(e["pair"], e["track"], e["velocity"]) for e in line["objects"]] for line in run["objects"]]

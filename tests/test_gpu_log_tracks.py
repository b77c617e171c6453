"""GPU, end to end: run_stream --cluster dbscan --tracks-log FILE --objects FILE2 on a synthetic log of six consecutive
frame-pair files (icp_flow_amd.synthetic.make_log; tests/test_carry.py shows the log to be what it claims).  The driver's ids,
carry counts and table against the restatement (tests/carry_restatement.py) run on the labels, pairs and object rows the same
run left; one id per object over the log; the braking box rough, the others smooth; four in flight byte for byte; a pose 5 m
off breaks the chain once."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carry_restatement as cr                 # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FILES = 6
DEV = torch.device("cuda:0")


def _write(root, pairs):
    os.makedirs(root)
    for k, pair in enumerate(pairs):
        np.savez(os.path.join(root, f"file_{k:02d}.npz"), **pair)
    return root


def _restate(recorded, radius=cr.CARRY_RADIUS, min_share=cr.CARRY_MIN_SHARE):
    """the chain of the log in numpy, on what the registrations left: per file the carry, the extension on the source side and
    the ids of the destination rows; then the table"""
    from icp_flow_amd import frame_pairs, synthetic as sy
    last, next_id, obs, carry, extend, poses = None, 0, [], [], [], []
    for fp, out in recorded:
        rows, _, ld = frame_pairs._frame_objects_device(fp, out, DEV, sy.LOG_SWEEP_SECONDS, 0.5)
        rows, ld, ls, pairs = rows.cpu().numpy(), ld.cpu().numpy(), out["labels_src"].cpu().numpy(), out["pairs"].cpu().numpy()
        if last is None:
            prior, counts = np.full(len(ls), -1, np.int32), np.zeros(6, np.int64)
        else:
            got = cr.rows_carry(last[0], last[1], fp.pose_exact, fp.points_src, radius, min_share)
            prior, counts = got["id"], got["counts"]
        want = cr.extend_side(ls, prior, next_id, rows, 0, 0, sy.LOG_SWEEP_SECONDS)
        next_id = want["next_id"]
        ids, _ = cr.pair_row_ids(ld, pairs, 1, want["obs"][:, 0].astype(np.int32), rows[:, 22])
        last = (fp.points_dst, ids)
        obs.append(want["obs"]), carry.append(counts), extend.append(want["counts"]), poses.append(fp.pose_exact)
    frames = cr.frames_chain(poses)
    step = np.repeat(np.arange(len(obs)), [len(o) for o in obs])
    table, counts = cr.path(np.concatenate(obs), step, frames, next_id)
    return dict(obs=obs, carry=carry, extend=extend, frames=frames, table=table, counts=counts, next_id=next_id)


def _run(directory, root, name, **kw):
    from icp_flow_amd import frame_pairs, synthetic as sy
    a = frame_pairs.default_args(**sy.LOG_CLUSTER)
    a.tracks_log, a.objects, a.sweep_seconds = str(root / f"log_{name}.jsonl"), str(root / f"objects_{name}.jsonl"), sy.LOG_SWEEP_SECONDS
    summary = frame_pairs.run_stream(a, frame_pairs.list_frame_pairs(directory), DEV, **kw)
    return dict(summary=summary, log=open(a.tracks_log, "rb").read(), tracks=[json.loads(line) for line in open(a.tracks_log)],
                objects=[json.loads(line) for line in open(a.objects)])


@pytest.fixture(scope="module")
def end_to_end(tmp_path_factory):
    from icp_flow_amd import frame_pairs, synthetic as sy
    root = tmp_path_factory.mktemp("log")
    pairs, truth = sy.make_log(0, FILES)
    directory = _write(str(root / "files"), pairs)
    recorded = []

    def register(args, fp, device):
        out = frame_pairs.register_frame_pair(args, fp, device)
        recorded.append((fp, out))
        return out

    serial = _run(directory, root, "serial", register_fn=register)
    flight = _run(directory, root, "in_flight", in_flight=4)
    plain_args = frame_pairs.default_args(**sy.LOG_CLUSTER)
    plain_args.objects, plain_args.sweep_seconds = str(root / "objects_plain.jsonl"), sy.LOG_SWEEP_SECONDS
    plain = frame_pairs.run_stream(plain_args, frame_pairs.list_frame_pairs(directory), DEV)
    # the second log: file 3's pose 5 m off (its points stay)
    off = [dict(p) for p in pairs]
    off[3]["pose"] = off[3]["pose"].copy()
    off[3]["pose"][1, 3] += 5.0
    broken_recorded = []

    def register_broken(args, fp, device):
        out = frame_pairs.register_frame_pair(args, fp, device)
        broken_recorded.append((fp, out))
        return out

    broken = _run(_write(str(root / "files_off"), off), root, "broken", register_fn=register_broken)
    return dict(truth=truth, recorded=recorded, serial=serial, flight=flight, plain=plain, plain_objects=open(plain_args.objects, "rb").read(),
                objects_serial=open(str(root / "objects_serial.jsonl"), "rb").read(), want=_restate(recorded), broken=broken,
                broken_want=_restate(broken_recorded))


def _object_of(recorded, truth, k, label_src):
    """the true object of a source cluster of file k: what most of its rows are"""
    fp, out = recorded[k]
    mine = truth["ids_src"][k][out["labels_src"].cpu().numpy() == F(label_src)]
    values, counts = np.unique(mine, return_counts=True)
    assert counts.max() == len(mine)                          # a cluster is one object, every row of it
    return int(values[np.argmax(counts)])


def test_the_drivers_ids_counts_and_table_equal_the_restatement(end_to_end):
    from icp_flow_amd import pair_judges, utils_tracks, synthetic as sy
    want, serial = end_to_end["want"], end_to_end["serial"]
    fps, outs = [r[0] for r in end_to_end["recorded"]], [r[1] for r in end_to_end["recorded"]]
    seen = pair_judges.log_tracks(fps, outs, DEV, sweep_seconds=sy.LOG_SWEEP_SECONDS)
    assert seen.next_id == want["next_id"] and np.array_equal(seen.path_counts[1:], want["counts"][1:]) and seen.path_counts[0] == want["next_id"]
    for k in range(FILES):
        assert np.array_equal(seen.carry_counts[k], want["carry"][k]), (k, seen.carry_counts[k], want["carry"][k])
        assert np.array_equal(seen.extend_counts[k], want["extend"][k]), (k, seen.extend_counts[k], want["extend"][k])
        assert np.array_equal(seen.observations[k], want["obs"][k]), k
    assert np.array_equal(seen.rows, want["table"]) and np.array_equal(seen.frames, want["frames"])
    # the driver: its file is that table as dicts (json round-trips a float64), its object lines carry the observations' ids
    restated = utils_tracks.LogTracks(want["table"], want["counts"], want["next_id"], want["obs"], want["carry"], want["extend"], want["frames"],
                                      [fp.name for fp in fps], [len(fp.points_src) for fp in fps], {})
    assert serial["tracks"] == restated.as_list()
    block = serial["summary"]["tracks_log"]
    assert {k: block[k] for k in restated.summary()} == restated.summary()
    for k, line in enumerate(serial["objects"]):
        assert [e["log_track"] for e in line["objects"]] == [int(want["obs"][k][e["pair"], 0]) for e in line["objects"]]
    assert (block["radius"], block["min_share"], block["max_dv"], block["min_speed"], block["min_iou"], block["sweep_seconds"]) == (0.02, 0.5, 1.0, 0.5, 0.5, 0.1)
    assert serial["summary"]["ms_tracks_log_per_file"] > 0 and serial["summary"]["tracks_log_file"].endswith("log_serial.jsonl")


def test_every_object_keeps_one_id_and_the_verdicts_are_the_scenes(end_to_end):
    """The mean velocity of every constant-velocity box is held against the truth at 4 x the largest deviation of the per-pair
    `velocity` of --objects in the same run (turned into the log's frame): the table's mean is (sum of R d) / (sum of seconds) at
    equal seconds, the average of the per-pair velocities, and cannot lie farther from the truth than the worst of them.  Measured
    on an MI355X: see COVERAGE.md row 19."""
    from icp_flow_amd import synthetic as sy
    truth, recorded, serial, want = end_to_end["truth"], end_to_end["recorded"], end_to_end["serial"], end_to_end["want"]
    track_of, per_pair = {}, 0.0
    for k, line in enumerate(serial["objects"]):
        R = want["frames"][k, :9].reshape(3, 3)
        here = {}
        for e in line["objects"]:
            j = _object_of(recorded, truth, k, e["label_src"])
            assert j >= 0 and e["log_track"] >= 0 and j not in here
            here[j] = e["log_track"]
            assert track_of.setdefault(j, e["log_track"]) == e["log_track"], (k, j)       # ONE id from its first file to its last
            if j != sy.LOG_BRAKING:
                per_pair = max(per_pair, float(np.linalg.norm(R @ np.asarray(e["velocity"]) - truth["velocity"][j, k])))
        assert sorted(here) == [j for j in range(len(sy.LOG_SIZES)) if truth["seen"][j, k]]                   # every object of the file, once
    assert len(set(track_of.values())) == len(track_of) == len(sy.LOG_SIZES)                                 # distinct objects, distinct ids
    by_id = {t["track"]: t for t in serial["tracks"]}
    assert sorted(by_id) == sorted(track_of.values())
    mean = 0.0
    for j, tid in track_of.items():
        t = by_id[tid]
        first = sy.LOG_LATE_FILE if j == sy.LOG_LATE else 0
        assert (t["first_step"], t["last_step"], t["counted"], t["missing"]) == (first, FILES - 1, FILES - first, 0) and t["judged"], (j, t)
        assert [o["step"] for o in t["observations"]] == list(range(first, FILES))
        assert t["smooth"] == (j != sy.LOG_BRAKING) and t["moving"] == (j != sy.LOG_WALL), (j, t)
        if j == sy.LOG_BRAKING:
            assert 2.0 < t["dv_max"] < 4.0                     # it loses 3 m/s between files 2 and 3
        else:
            mean = max(mean, float(np.linalg.norm(np.asarray(t["velocity"]) - truth["velocity"][j, 0])))
            assert t["dv_max"] < 0.5
    print(f"per-pair velocity off by {per_pair:.6f} m/s at most, the tracks' mean velocity by {mean:.6f} m/s at most")
    assert mean <= 4 * per_pair
    block = serial["summary"]["tracks_log"]
    assert {k: block[k] for k in ("files", "tracks", "observed", "judged", "smooth", "rough", "moving", "breaks", "overflow")} == dict(
        files=FILES, tracks=6, observed=6, judged=6, smooth=5, rough=1, moving=5, breaks=0, overflow=0)
    assert 0 < block["carried_rows"] < block["rows"] == sum(len(fp.points_src) for fp, _ in recorded[1:])


def test_four_in_flight_give_the_same_file_and_the_other_keys_stay(end_to_end):
    serial, flight, plain = end_to_end["serial"], end_to_end["flight"], end_to_end["plain"]
    assert flight["log"] == serial["log"] and len(serial["log"]) > 0                  # byte for byte
    assert flight["summary"]["tracks_log"] == serial["summary"]["tracks_log"]
    new = ["tracks_log", "ms_tracks_log_per_file", "tracks_log_file"]
    assert [k for k in serial["summary"] if k not in plain] == new
    timing = ("ms_per_frame_pair", "frame_pairs_per_s", "ms_objects_per_frame_pair", "objects_file")
    assert {k: v for k, v in serial["summary"].items() if k in plain and k not in timing} == {k: v for k, v in plain.items() if k not in timing}
    # the objects' file without the judge: the same lines, less `log_track`
    stripped = [dict(line, objects=[{k: v for k, v in e.items() if k != "log_track"} for e in line["objects"]]) for line in serial["objects"]]
    assert "".join(json.dumps(line) + "\n" for line in stripped).encode() == end_to_end["plain_objects"]


def test_a_pose_5_m_off_breaks_the_chain_once(end_to_end):
    broken, want = end_to_end["broken"], end_to_end["broken_want"]
    block = broken["summary"]["tracks_log"]
    assert block["breaks"] == 1 and [int(c[5]) for c in want["carry"]] == [0, 0, 0, 1, 0, 0]           # exactly one break, at step 3
    assert want["carry"][3][0] < 0.05 * sum(want["carry"][3][[0, 2]])
    before = {e["log_track"] for line in broken["objects"][:3] for e in line["objects"]}
    after = {e["log_track"] for line in broken["objects"][3:] for e in line["objects"]}
    assert min(before | after) >= 0 and not (before & after)                          # fresh ids from there on, no id used twice
    assert len(before) == 6 and len(after) == 6 and block["tracks"] == 12 and block["observed"] == 12
    for line in broken["objects"]:
        ids = [e["log_track"] for e in line["objects"]]
        assert len(set(ids)) == len(ids)
    for k, line in enumerate(broken["objects"]):
        assert [e["log_track"] for e in line["objects"]] == [int(want["obs"][k][e["pair"], 0]) for e in line["objects"]]
    steps = {t["track"]: (t["first_step"], t["last_step"]) for t in broken["tracks"]}
    assert all(steps[i][1] <= 2 for i in before) and all(steps[i][0] >= 3 for i in after)

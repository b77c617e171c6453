"""GPU: the object tracks (icpflow_label_overlap, icpflow_object_tracks_extend, icpflow_object_tracks_fit; csrc/overlap.hip,
csrc/tracks.hip) against their numpy restatement (tests/track_restatement.py), np.array_equal with NaN = NaN throughout: every
call on an exactly sized, 0xFF-filled workspace between guards, every output poisoned between guards, every word of the rows
before a table's number written and none behind it (tests/track_device.py); a rerun and a second stream bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_cases as tc                       # noqa: E402
import track_restatement as trk                # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def td():
    import track_device
    return track_device


# ---------------------------------------------------------------------------------------------------------------- overlap

@pytest.mark.parametrize("n", tc.SIZES)
def test_overlap_of_random_labellings_at_every_size(td, n):
    a, b = tc.random_pair(n, 100 + n)
    ta, tb, counts, _ = td.check_overlap(a, b, Lmax=16, label=f"n={n}")
    if n == 0:
        assert len(ta) == 0 and len(tb) == 0 and not counts.any()


@pytest.mark.parametrize("cuts", tc.LONG_CUTS)
def test_a_segment_of_three_chunks_split_over_three_partners(td, cuts):
    a, b = tc.long_segment(cuts)
    ta, tb, counts, _ = td.check_overlap(a, b, Lmax=8, label=str(cuts))
    sizes = [cuts[0], cuts[1] - cuts[0], 2049 - cuts[1]]
    row = ta[2]                                           # labels -1e8, 2, 5
    assert (row[0], row[1], row[2]) == (5.0, 2049, 2049)
    best = int(np.argmax(sizes))
    assert row[3] == 1 + best and row[5] == max(sizes) and row[6] == sorted(sizes)[1]
    assert tb[1:4, 5].tolist() == sizes and tb[1:4, 3].tolist() == [2, 2, 2]
    assert counts.tolist() == [2349, 2, 2, 4]


def test_4096_segments_a_side(td):
    a, b = tc.many_segments()
    ta, tb, counts, _ = td.check_overlap(a, b, Lmax=4096, label="many")
    assert len(ta) == 4096 and len(tb) == 4096 and counts[0] == 8192 and counts[2] == 4096 and counts[3] == 4096
    assert (ta[:, 5] == 1).all() and (ta[:, 6] == 1).all()          # every partner a tie of 1 : 1


def test_4097_labels_on_one_side_leave_the_tables_untouched(td):
    a, b = np.arange(4097, dtype=F), np.zeros(4097, F)
    for x, y, want in ((a, b, (-4097, 1)), (b, a, (1, -4097))):
        ta, tb, num_a, num_b, counts, _ = td.run_overlap(x, y, Lmax=4096)   # (run_overlap asserts the poison of both tables)
        assert (num_a, num_b) == want and len(ta) == 0 and len(tb) == 0 and not counts.any()
    ta, tb, num_a, num_b, counts, _ = td.run_overlap(a[:9], b[:9], Lmax=8)
    assert (num_a, num_b) == (-9, 1) and not counts.any()


def test_special_labels(td):
    a, b = tc.special_labels()
    ta, tb, _, _ = td.check_overlap(a, b, Lmax=16, label="special")
    assert len(ta) == 10 and len(tb) == 10                 # both zeros one label, the three NaNs apart
    assert np.isnan(ta[0, 0])                              # a NaN with the sign bit sorts before -inf, and is no negative number
    assert ta[1:4, 0].tolist() == [-np.inf, -1e8, -1.0] and (ta[1:4, 3] == -1).all() and not ta[1:4, [2, 4, 5, 6, 7, 8, 9]].any()
    assert ta[4:8, 0].tolist() == [0.0, 2.5, 1e7, np.inf] and np.isnan(ta[8:, 0]).all()
    linkable = [0, 4, 5, 6, 7, 8, 9]
    assert np.isin(ta[linkable, 3], linkable).all() and np.isin(tb[linkable, 3], linkable).all()


def test_ties_go_to_the_lower_index_and_decide_mutual(td):
    ta, tb, _, _ = td.check_overlap(*tc.tie_two_two(), Lmax=4, label="2:2")
    assert ta[1, 0] == 7 and (ta[1, 3], ta[1, 4], ta[1, 5], ta[1, 6]) == (0, 1.0, 2, 2)
    ta, tb, counts, _ = td.check_overlap(*tc.tie_mutual(), Lmax=4, label="mutual")
    assert ta[:, 3].tolist() == [0, 0] and tb[:, 3].tolist() == [0, 0]
    assert ta[:, 8].tolist() == [1, 0] and tb[:, 8].tolist() == [1, 0] and counts.tolist() == [4, 1, 2, 2]


def test_a_segment_whose_rows_are_all_negative_on_the_other_side(td):
    ta, tb, counts, _ = td.check_overlap(*tc.all_negative_other_side(), Lmax=4, label="negative")
    assert ta[1].tolist() == [3.0, 3, 0, -1, 0, 0, 0, 0, 0, 0] and ta[2, 3] == 3 and ta[2, 9] == 2 / 3
    assert counts.tolist() == [2, 1, 1, 1]


def test_identical_permuted_and_constant_labellings(td):
    a, perm = tc.relabelled()
    ta, tb, counts, _ = td.check_overlap(a, a, Lmax=16, label="identical")
    assert (ta[:, 9] == 1).all() and (ta[:, 8] == 1).all() and (ta[:, 3] == np.arange(9)).all() and counts.tolist() == [500, 9, 9, 9]
    ta, tb, counts, _ = td.check_overlap(a, perm, Lmax=16, label="permuted")
    assert (ta[:, 9] == 1).all() and (ta[:, 8] == 1).all() and sorted(ta[:, 3].tolist()) == list(range(9))
    ta, tb, counts, _ = td.check_overlap(a, np.full(500, 4.0, F), Lmax=16, label="constant")
    assert len(tb) == 1 and (ta[:, 3] == 0).all() and ta[:, 8].sum() == 1 and counts.tolist() == [500, 1, 9, 1]
    td.check_overlap(a, np.full(500, -1.0, F), Lmax=16, label="all noise")


def test_overlap_is_bit_identical_on_a_rerun_and_on_a_second_stream(td):
    a, b = tc.long_segment(tc.LONG_CUTS[0])
    first = td.run_overlap(a, b, Lmax=8)[-1]
    assert td.run_overlap(a, b, Lmax=8)[-1] == first
    assert td.run_overlap(a, b, Lmax=8, stream=torch.cuda.Stream())[-1] == first


# --------------------------------------------------------------------------------------------------------------- extension

def _objects_of(step):
    """one object row per label of the gap, one for a label that is no segment, one without a box, one on the noise"""
    labels = sorted(set(step["labels"].tolist()) - {-1.0})
    rows = [tc.object_row(lab, d=(0.5 * k, 0.25, 0.0), size=(2.0 + k, 3.0, 1.5), points=10 + k) for k, lab in enumerate(labels)]
    return np.array(rows + [tc.object_row(999.0), tc.object_row(labels[0], points=0), tc.object_row(-1.0)])


def test_the_hand_made_chain_of_three_gaps(td):
    state, next_id = np.full(tc.CHAIN_ROWS, -1, np.int32), 0
    for gap, step in enumerate(tc.chain(), start=1):
        objects = _objects_of(step)
        got = td.check_extend(step["labels"], state, next_id, objects, gap, 0.1 * gap, label=f"gap {gap}")
        assert got["track_of_row"].tolist() == step["ids"].tolist() and got["next_id"] == step["next_id"]
        assert got["segments"][:, 2].tolist() == step["segment_ids"] and got["segments"][:, 3].tolist() == step["inherited"]
        assert got["obs"][-3:, 0].tolist() == [-1, -1, -1] and got["obs"][:-3, 0].tolist() == step["segment_ids"][1:]
        assert got["counts"][3:].tolist() == [len(objects) - 3, 3, 0]
        state, next_id = got["track_of_row"], got["next_id"]
    assert got["segments"][2, 4:6].tolist() == [2, 0.5]     # IoU exactly min_iou: `>=`


def test_an_iou_one_step_below_min_iou_founds_a_track(td):
    steps = tc.chain()
    got = td.check_extend(steps[2]["labels"], steps[1]["ids"], 7, None, 3, 0.3, min_iou=np.nextafter(0.5, 1.0), label="above")
    assert got["segments"][:, 2].tolist() == [-1, 4, 7] and got["next_id"] == 8 and got["counts"].tolist() == [2, 1, 1, 0, 0, 0]
    assert got["track_of_row"][23:26].tolist() == [7, 7, 7] and len(got["obs"]) == 0        # P = 0


def test_extension_of_nothing_and_of_noise_alone(td):
    got = td.check_extend(np.zeros(0, F), np.zeros(0, np.int32), 5, [tc.object_row(1.0)], 1, 0.1, label="n = 0")
    assert got["num"] == 0 and got["next_id"] == 5 and got["obs"][0, 0] == -1
    got = td.check_extend(np.full(70, -1.0, F), np.full(70, -1, np.int32), 0, None, 1, 0.1, label="noise")
    assert got["num"] == 1 and got["next_id"] == 0 and (got["track_of_row"] == -1).all()


def test_overflow_leaves_the_state_bit_for_bit(td):
    state = (np.arange(40, dtype=np.int32) % 7) - 1
    for labels, st, nid, name in ((np.arange(40, dtype=F), state, 9, "labels"),                       # 40 labels, Lmax 16
                                  (np.zeros(40, F), np.arange(40, dtype=np.int32), 40, "ids"),         # 40 live ids
                                  (np.arange(40, dtype=F) % 5, state, (1 << 24) - 3, "id range")):     # 5 fresh ids beyond 2^24
        got = td.check_extend(labels, st, nid, [tc.object_row(1.0)], 2, 0.2, Lmax=16, label=name)
        assert got["num"] < 0 and got["next_id"] == nid and np.array_equal(got["track_of_row"], st), name
        assert got["counts"].tolist() == [0, 0, 0, 0, 1, 1] and got["obs"][0, 0] == -1 and len(got["segments"]) == 0


def test_extension_is_bit_identical_on_a_rerun_and_on_a_second_stream(td):
    steps = tc.chain()
    args = (steps[1]["labels"], steps[0]["ids"], 6, _objects_of(steps[1]), 2, 0.2)
    first = td.run_extend(*args)["raw"]
    assert td.run_extend(*args)["raw"] == first and td.run_extend(*args, stream=torch.cuda.Stream())["raw"] == first


def test_a_larger_random_chain_follows_the_restatement(td):
    """2500 rows, three chunks in the largest cluster, labels that split, merge and vanish from gap to gap"""
    rng = np.random.default_rng(8)
    base = np.repeat(np.arange(6), [2100, 150, 100, 70, 50, 30])
    state, next_id = np.full(2500, -1, np.int32), 0
    for gap in (1, 2, 3):
        labels = base.astype(F) * 2.0 + (rng.random(2500) < 0.2 * (gap - 1)) * 1.0     # a fifth, two fifths of every cluster split off
        labels[rng.random(2500) < 0.1] = -1.0
        got = td.check_extend(labels, state, next_id, None, gap, 0.1 * gap, Lmax=32, label=f"random gap {gap}")
        state, next_id = got["track_of_row"], got["next_id"]
    assert next_id > 6


# --------------------------------------------------------------------------------------------------------------------- fit

def test_one_observation_is_not_judged(td):
    tracks, counts, _ = td.check_fit([tc.observation(0, 1, 0.125, (0.25, 0.0, 0.0))], 1)
    assert tracks[0, 1] == 1 and tracks[0, 2] == 2 and tracks[0, 3] == 2.0 and tracks[0, 7] == 0 and tracks[0, 9:12].tolist() == [1, 0, 0]
    assert counts.tolist() == [1, 1, 0, 0, 1]
    tracks, counts, _ = td.check_fit([tc.observation(0, 1, 0.1, (0.2, 0.0, 0.0))] * 2, 1)     # twice in ONE gap: still not judged
    assert tracks[0, 1] == 2 and tracks[0, 10] == 0


def test_two_gaps_exactly_on_a_line_have_residual_zero(td):
    """s = 0.125, 0.25 and d = s v with v = (2, -4, 0.5): every product, sum and quotient is exact in binary"""
    obs = [tc.observation(1, g, 0.125 * g, (0.25 * g, -0.5 * g, 0.0625 * g)) for g in (1, 2)]
    tracks, counts, _ = td.check_fit(obs, 2)
    assert tracks[1, 3:6].tolist() == [2.0, -4.0, 0.5] and tracks[1, 7] == 0.0 and tracks[1, 8] == 0.0 and tracks[1, 9:12].tolist() == [1, 1, 1]
    assert tracks[1, 2] == 6 and tracks[0].tolist() == [0.0] * 16        # a track with no observation: its id and zeros
    assert counts.tolist() == [2, 1, 1, 1, 1]


@pytest.mark.parametrize("side", (-1, 0, 1))
def test_the_largest_residual_one_step_either_side_of_max_residual(td, side):
    """d = (+x, 0) and (-x, 0) at equal s in two gaps: v = 0 exactly, both residuals sqrt(x * x) = x exactly (a correctly rounded
    root of a correctly rounded square gives |x| back in binary floating point)"""
    x = 0.2 if side == 0 else np.nextafter(0.2, side * np.inf)
    obs = [tc.observation(0, 1, 0.5, (x, 0.0, 0.0)), tc.observation(0, 2, 0.5, (-x, 0.0, 0.0))]
    tracks, counts, _ = td.check_fit(obs, 1, max_residual=0.2)
    assert tracks[0, 7] == x and tracks[0, 10] == 1 and tracks[0, 11] == (1.0 if side <= 0 else 0.0)


def test_no_tracks_and_no_observations(td):
    tracks, counts, _ = td.check_fit(np.zeros((0, 13)), 0)
    assert tracks.shape == (0, 16) and counts.tolist() == [0, 0, 0, 0, 0]
    tracks, counts, _ = td.check_fit([tc.observation(-1, 1, 0.1, (1.0, 0.0, 0.0))], 0)
    assert counts.tolist() == [0, 0, 0, 0, 0]
    tracks, counts, _ = td.check_fit(np.zeros((0, 13)), 300)
    assert (tracks[:, 0] == np.arange(300)).all() and not tracks[:, 1:].any() and counts.tolist() == [300, 0, 0, 0, 0]


def test_many_tracks_sizes_and_a_rerun(td):
    rng = np.random.default_rng(11)
    obs = []
    for g in (1, 2, 3):
        for t in rng.permutation(300)[:250]:
            obs.append(tc.observation(int(t), g, 0.1 * g, rng.normal(0, 1, 3) * 0.1 * g, size=rng.random(3) * 5, points=int(rng.integers(1, 500))))
        obs.append(tc.observation(-1, g, 0.1 * g, (9.0, 9.0, 9.0)))
    tracks, counts, raw = td.check_fit(obs, 300)
    assert counts[0] == 300 and 250 <= counts[1] <= 300
    assert td.run_fit(obs, 300)[2] == raw and td.run_fit(obs, 300, stream=torch.cuda.Stream())[2] == raw


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_the_device_wrappers_give_what_the_raw_calls_give(td):
    from icp_flow_amd import utils_tracks
    a, b = tc.random_pair(1500, 77)
    ta, na, tb, nb, counts = utils_tracks.label_overlap_device(td.upload(a, F), td.upload(b, F), Lmax=16)
    wa, wb, wna, wnb, wcounts = trk.label_overlap(a, b, 16)
    assert (int(na), int(nb)) == (wna, wnb) and np.array_equal(counts.cpu().numpy(), wcounts)
    td.same(ta[:wna].cpu().numpy(), wa, "A")
    td.same(tb[:wnb].cpu().numpy(), wb, "B")
    state = utils_tracks.TrackState(tc.CHAIN_ROWS, td.DEV, Lmax=16)
    want_state, want_next, want_obs = np.full(tc.CHAIN_ROWS, -1, np.int32), 0, []
    for gap, step in enumerate(tc.chain(), start=1):
        objects = _objects_of(step)
        state.extend(td.upload(step["labels"], F), td.upload(objects, np.float64), gap, 0.1 * gap)
        want = trk.extend(step["labels"], want_state, want_next, objects, gap, 0.1 * gap, Lmax=16)
        want_state, want_next = want["track_of_row"], want["next_id"]
        want_obs.append(want["obs"])
    tracks = state.read()
    rows, counts = trk.fit(np.concatenate(want_obs), want_next)
    assert tracks.next_id == want_next == 7 and np.array_equal(state.track_of_row.cpu().numpy(), want_state)
    td.same(tracks.rows, rows, "tracks")
    assert tracks.fit_counts[1:].tolist() == counts[1:].tolist() and tracks.fit_counts[0] == state.bound == 48
    assert [i.tolist() for i in tracks.observation_ids] == [o[:, 0].astype(int).tolist() for o in want_obs]
    assert tracks.summary()["tracks"] == 7 and tracks.summary()["overflow"] == 0


# ------------------------------------------------------------------------------------------------------------------ end to end

@pytest.fixture(scope="module")
def end_to_end(tmp_path_factory):
    """run_stream over the scene's sequence file, --cluster dbscan, --tracks FILE --objects FILE: once frame pair by frame pair
    (every registration recorded), once with four in flight"""
    import json
    from icp_flow_amd import frame_pairs
    root = tmp_path_factory.mktemp("tracks")
    path = str(root / "sample.npz")
    np.savez(path, **tc.scene()["arrays"])
    recorded = []

    def register(args, fp, device):
        out = frame_pairs.register_frame_pair(args, fp, device)
        recorded.append((fp, out))
        return out

    runs = {}
    for name, kw in (("serial", dict(register_fn=register)), ("in_flight", dict(in_flight=4))):
        a = frame_pairs.default_args(**tc.SCENE_CLUSTER)
        a.tracks, a.objects, a.sweep_seconds = str(root / f"tracks_{name}.jsonl"), str(root / f"objects_{name}.jsonl"), tc.SCENE_SWEEP_SECONDS
        summary = frame_pairs.run_stream(a, [path], td_dev(), **kw)
        runs[name] = dict(summary=summary, tracks=[json.loads(line) for line in open(a.tracks)], objects=[json.loads(line) for line in open(a.objects)])
    plain = frame_pairs.run_stream(frame_pairs.default_args(**tc.SCENE_CLUSTER), [path], td_dev())
    return dict(path=path, recorded=recorded, plain=plain, **runs)


def td_dev():
    return torch.device("cuda:0")


def test_end_to_end_the_tracks_equal_the_restatement_on_what_the_run_left(end_to_end):
    from icp_flow_amd import frame_pairs, utils_tracks
    recorded = end_to_end["recorded"]
    assert [fp.gap for fp, _ in recorded] == [1, 2, 3]
    state, next_id, obs = np.full(len(recorded[0][0].points_dst), -1, np.int32), 0, []
    for fp, out in recorded:
        seconds = fp.gap * tc.SCENE_SWEEP_SECONDS
        rows, _, labels = frame_pairs._frame_objects_device(fp, out, td_dev(), seconds, 0.5)
        want = trk.extend(labels.cpu().numpy(), state, next_id, rows.cpu().numpy(), fp.gap, seconds)
        assert want["counts"][5] == 0
        state, next_id = want["track_of_row"], want["next_id"]
        obs.append(want["obs"])
    rows, counts = trk.fit(np.concatenate(obs), next_id)
    want = utils_tracks.Tracks(rows, counts, next_id, [1, 2, 3], [o[:, 0] for o in obs], [np.zeros(6)] * 3, {})
    line = end_to_end["serial"]["tracks"]
    assert len(line) == 1 and line[0]["path"] == end_to_end["path"] and line[0]["gaps"] == [1, 2, 3] and line[0]["frame_pairs"] == [0, 1, 2]
    assert line[0]["tracks"] == want.as_list()                        # every number bit for bit (json round-trips a float64)
    assert line[0]["observations"] == [i.tolist() for i in want.observation_ids]
    got = line[0]["counts"]
    assert {k: got[k] for k in ("tracks", "observed", "judged", "consistent", "moving")} == {k: want.summary()[k] for k in ("tracks", "observed", "judged", "consistent", "moving")}


def test_end_to_end_the_counts_are_the_scenes_and_the_velocities_the_truth(end_to_end):
    """Five tracks seen in all three gaps, four consistent, one not, four moving (the wall stands).  The fitted velocities are held
    against the truth at 4 x the largest deviation of the per-pair `velocity` of --objects (the parent's code) in the same run: a
    fitted velocity is a convex combination (weights s^2) of its track's per-pair velocities, so it cannot lie farther from the
    truth than the worst of them.  Measured on an MI355X: per-pair 0.003447 m/s at most, fitted 0.001360 m/s at most; residuals
    of the four consistent tracks 0.000346 m at most, of the bad one 0.428 m: 0.2 m lies far from both."""
    line, summary = end_to_end["serial"]["tracks"][0], end_to_end["serial"]["summary"]
    tracks = line["tracks"]
    assert len(tracks) == 5 and all(t["gaps"] == [1, 2, 3] and t["observations"] == 3 and t["judged"] for t in tracks)
    truth = tc.scene_truth_velocity()
    speeds = np.linalg.norm(truth[:, :2], axis=1)

    def obj_of(v):                                                     # the object a velocity belongs to: the nearest truth
        return int(np.argmin(np.linalg.norm(truth - np.asarray(v), axis=1)))

    per_pair, objects_of_track = 0.0, {}
    for pair_line in end_to_end["serial"]["objects"]:
        for e in pair_line["objects"]:
            assert e["track"] >= 0
            k = objects_of_track.setdefault(e["track"], obj_of(e["velocity"]))
            if not (k == tc.SCENE_BAD and pair_line["frame_pair"] == tc.SCENE_BAD_FRAME - 1):
                per_pair = max(per_pair, float(np.linalg.norm(np.asarray(e["velocity"]) - truth[k])))
    assert sorted(objects_of_track.values()) == [0, 1, 2, 3, 4]        # one track per object, the same over the three gaps
    fitted, residual_good = 0.0, 0.0
    for t in tracks:
        k = objects_of_track[t["track"]]
        assert t["consistent"] == (k != tc.SCENE_BAD) and t["moving"] == (speeds[k] >= 0.5), (k, t)
        if k != tc.SCENE_BAD:
            fitted = max(fitted, float(np.linalg.norm(np.asarray(t["velocity"]) - truth[k])))
            residual_good = max(residual_good, t["residual_max"])
        else:
            residual_bad = t["residual_max"]
    print(f"per-pair velocity off by {per_pair:.6f} m/s at most, fitted by {fitted:.6f}; residuals {residual_good:.6f} m, bad {residual_bad:.6f} m")
    assert fitted <= 4 * per_pair
    assert residual_good < 0.2 / 4 and residual_bad > 0.2 * 2           # the policy sits far from both sides
    block = summary["tracks"]
    assert {k: block[k] for k in ("samples", "tracks", "observed", "judged", "consistent", "inconsistent", "moving", "overflow")} == dict(
        samples=1, tracks=5, observed=5, judged=5, consistent=4, inconsistent=1, moving=4, overflow=0)
    assert (block["min_iou"], block["max_residual"], block["min_speed"], block["sweep_seconds"]) == (0.5, 0.2, 0.5, tc.SCENE_SWEEP_SECONDS)
    assert summary["ms_tracks_per_sample"] > 0 and summary["tracks_file"].endswith("tracks_serial.jsonl")
    sizes = {objects_of_track[t["track"]]: t["size"] for t in tracks}
    assert all(abs(sizes[k][0] - tc.SCENE_SIZES[k][0]) < 0.15 and abs(sizes[k][2] - tc.SCENE_SIZES[k][2]) < 0.15 for k in range(5))


def test_end_to_end_four_in_flight_give_the_same_tracks_and_the_summary_stays(end_to_end):
    serial, flight, plain = end_to_end["serial"], end_to_end["in_flight"], end_to_end["plain"]
    assert flight["tracks"] == serial["tracks"]
    assert [[e["track"] for e in line["objects"]] for line in flight["objects"]] == [[e["track"] for e in line["objects"]] for line in serial["objects"]]
    assert {k: v for k, v in flight["summary"]["tracks"].items()} == serial["summary"]["tracks"]
    new = ["objects", "ms_objects_per_frame_pair", "objects_file", "tracks", "ms_tracks_per_sample", "tracks_file"]
    assert [k for k in serial["summary"] if k not in plain] == new
    timing = ("ms_per_frame_pair", "frame_pairs_per_s")
    assert {k: v for k, v in serial["summary"].items() if k in plain and k not in timing} == {k: v for k, v in plain.items() if k not in timing}

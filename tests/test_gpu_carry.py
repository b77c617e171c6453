"""GPU: object tracks across the files of a log (include/icpflow_hip.h 8(l): icpflow_rows_carry, icpflow_pair_row_ids,
icpflow_object_tracks_extend_side, icpflow_object_tracks_path; csrc/carry.hip, csrc/tracks.hip) against their numpy restatement
(tests/carry_restatement.py), np.array_equal with NaN = NaN and the BITS of d2 throughout: every call on an exactly sized,
0xFF-filled workspace between guards, every output poisoned between guards (tests/carry_device.py); a rerun and a second stream
bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import carry_cases as cc                       # noqa: E402
import carry_restatement as cr                 # noqa: E402
import track_cases as tc                       # noqa: E402
import track_restatement as trk                # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
POSE_NAMES = tuple(cc.POSES)


@pytest.fixture(scope="module")
def cd():
    import carry_device
    return carry_device


# -------------------------------------------------------------------------------------------------------------------- the carry

@pytest.mark.parametrize("m", cc.SIZES)
def test_the_carry_at_every_pair_of_sizes(cd, m):
    """n and m over the grid's bucket-count steps and the seams of its scan tiles; the poses take turns"""
    for k, n in enumerate(cc.SIZES):
        name = POSE_NAMES[(k + cc.SIZES.index(m)) % 3]
        prev, prev_id, nxt = cc.views(n, m, 7 * n + m, cc.POSES[name])
        got, want = cd.check_carry(prev, prev_id, cc.POSES[name], nxt, cc.RADIUS, 0.0, label=f"n={n} m={m} {name}")
        assert got["counts"][5] == 0 and got["counts"][0] + got["counts"][2] == n
        if min(n, m) >= 512:
            assert got["counts"][0] > 0.5 * min(n, m) * min(n, m) / max(n, m) and got["counts"][2] > 0     # both hits and misses occur


@pytest.mark.parametrize("name", POSE_NAMES)
def test_the_carry_under_every_pose(cd, name):
    prev, prev_id, nxt = cc.views(2049, 2049, 11, cc.POSES[name])
    got, _ = cd.check_carry(prev, prev_id, cc.POSES[name], nxt, cc.RADIUS, 0.5, label=name)
    assert got["counts"][0] > 0.6 * 2049 and got["counts"][5] == 0 and (got["id"] >= 0).sum() == got["counts"][1] > 0
    cd.check_carry(prev, prev_id, cc.POSES[name], nxt, cc.RADIUS, 0.5, label=name + " ids alone", per_row=False)


def test_ties_go_to_the_lowest_previous_row(cd):
    prev, prev_id, nxt = cc.views(600, 300, 5, cc.POSES["yaw30"])
    prev = np.concatenate([prev, prev[::-1]])                  # every previous row twice: row j and row 599 - j
    ids = np.arange(600, dtype=np.int32)
    got, _ = cd.check_carry(prev, ids, cc.POSES["yaw30"], nxt, cc.RADIUS, 0.0, label="duplicates")
    assert (got["idx"][got["idx"] >= 0] < 300).all() and got["counts"][0] > 100
    # two previous rows at exactly equal d2 (dyadic, identity pose), the farther-listed decoys around them
    prev = np.array([[9, 9, 9], [1 / 128, 0, 0], [-1 / 128, 0, 0], [0, 1 / 128, 0], [0, 1 / 64, 0]], F)
    got, _ = cd.check_carry(prev, [0, 1, 2, 3, 4], np.eye(4), [[0, 0, 0], [0, 3 / 256, 0]], cc.RADIUS, 0.0, label="equal d2")
    assert got["idx"].tolist() == [1, 3] and got["d2"].tolist() == [(1 / 128) ** 2, (1 / 256) ** 2]


def test_a_query_exactly_at_the_radius_hits_and_one_step_beyond_misses(cd):
    hit, miss = cc.at_radius()
    got, _ = cd.check_carry([[0, 0, 0]], [7], np.eye(4), [[hit, 0, 0], [miss, 0, 0], [0, -hit, 0], [0, 0, miss]], cc.RADIUS, 0.0, label="r2")
    assert got["id"].tolist() == [7, -1, 7, -1] and got["counts"].tolist() == [2, 2, 2, 0, 0, 0]
    rf = F(cc.RADIUS)
    assert got["d2"][0] == hit * hit <= rf * rf and got["d2"][1] == rf * rf


def test_bad_rows_each_with_its_count(cd):
    prev, prev_id, nxt = cc.views(513, 513, 21, cc.POSES["yaw30"])
    prev[[3, 100]] = [[np.nan, 0, 0], [0, 0, np.inf]]
    prev[200:210] = 1e8                                         # pad rows
    nxt[[5, 6, 7]] = [[0, np.nan, 0], [1e8, 1e8, 1e8], [-np.inf, 0, 0]]
    got, _ = cd.check_carry(prev, prev_id, cc.POSES["yaw30"], nxt, cc.RADIUS, 0.0, label="bad rows")
    assert got["counts"][3] == 3 and got["counts"][4] == 12 and got["idx"][[5, 6, 7]].tolist() == [-2, -2, -2] and (got["id"][[5, 6, 7]] == -1).all()
    assert got["counts"][0] + got["counts"][2] + 3 == 513
    got, _ = cd.check_carry([[1e8, 1e8, 1e8]], [3], cc.rigid(45.0), [[0, 0, 0]], 1000.0, 0.0, label="a pad row the rotation cancels")
    assert got["counts"].tolist() == [0, 0, 1, 0, 1, 0]
    got, _ = cd.check_carry(prev, np.full(513, -1, np.int32), cc.POSES["yaw30"], nxt, cc.RADIUS, 0.5, label="no ids")
    assert got["counts"][1] == 0 and got["counts"][0] > 250 and got["counts"][5] == 0 and (got["id"] == -1).all()


def test_min_share_breaks_the_chain_one_hit_below_the_product_and_not_at_it(cd):
    targets = np.arange(10)[:, None] * np.array([[1.0, 0, 0]])
    for hits, share, broken in ((4, 0.5, 1), (5, 0.5, 0), (0, 0.0, 0), (10, 1.0, 0), (9, 1.0, 1), (4, 0.0, 0)):
        nxt = targets.copy()
        nxt[hits:, 1] = 3.0                                     # the rows from `hits` on lie 3 m off
        got, _ = cd.check_carry(targets, np.arange(10) + 20, np.eye(4), nxt, cc.RADIUS, share, label=f"{hits} hits, min_share {share}")
        assert got["counts"].tolist() == [hits, hits, 10 - hits, 0, 0, broken]
        assert got["id"].tolist() == ([-1] * 10 if broken else list(range(20, 20 + hits)) + [-1] * (10 - hits))
        assert got["idx"].tolist() == list(range(hits)) + [-1] * (10 - hits)          # what the search found stays, broken or not
    got, _ = cd.check_carry(np.zeros((0, 3)), [], np.eye(4), targets, cc.RADIUS, 0.5, label="m = 0")
    assert got["counts"].tolist() == [0, 0, 10, 0, 0, 1]
    got, _ = cd.check_carry(np.zeros((0, 3)), [], np.eye(4), targets, cc.RADIUS, 0.0, label="m = 0, min_share 0")
    assert got["counts"].tolist() == [0, 0, 10, 0, 0, 0]
    got, _ = cd.check_carry(targets, np.arange(10), np.eye(4), np.zeros((0, 3)), cc.RADIUS, 1.0, label="n = 0")
    assert got["counts"].tolist() == [0] * 6


def test_the_carry_is_bit_identical_on_a_rerun_and_on_a_second_stream(cd):
    prev, prev_id, nxt = cc.views(4097, 2049, 31, cc.POSES["far"])
    args = (prev, prev_id, cc.POSES["far"], nxt, cc.RADIUS, 0.5)
    first = cd.run_carry(*args)["raw"]
    assert cd.run_carry(*args)["raw"] == first and cd.run_carry(*args, stream=torch.cuda.Stream())["raw"] == first


# ----------------------------------------------------------------------------------------------------------------- the pair ids

@pytest.mark.parametrize("P", (0, 1, 1024, 1025, 4096))
def test_the_row_ids_at_every_number_of_pairs(cd, P):
    pool, rows, ids, weight = cc.pair_table(P, 40 + P, labels=200 if P > 1 else 2)
    rng = np.random.default_rng(P)
    for col, n, w, stride in ((0, 1024, None, 1), (1, 1025, weight, 1), (1, 2500, weight, 24), (0, 0, weight, 1)):
        labels = pool[rng.integers(0, len(pool), n)]
        got, counts, _ = cd.check_row_ids(labels, rows, col, ids, w, stride, label=f"P={P} col={col} n={n}")
        assert counts[0] + counts[1] == n
        if P == 0:
            assert (got == -1).all() and counts[2] == 0
        if P >= 1024:
            assert counts[2] > 0 and (n == 0 or counts[0] > 0)


def test_special_labels_weights_that_decide_and_ties(cd):
    rows = np.array([[1, 5], [2, 5], [3, 5], [4, -0.0], [5, cc.NAN_A], [6, -1.0], [-1e8, 7]], F)
    labels = np.array([5, 0.0, -0.0, cc.NAN_A, cc.NAN_B, cc.NAN_SIGNED, -1, -1e8, 6, 7], F)
    ids = [10, 11, 12, 13, 14, 15, 16]
    got, counts, _ = cd.check_row_ids(labels, rows, 1, ids, [1.0, 3.0, 2.0, 0, 0, 0, 0], label="weights decide")
    assert got.tolist() == [11, 13, 13, 14, -1, -1, -1, -1, -1, 16] and counts.tolist() == [5, 5, 2]
    got, _, _ = cd.check_row_ids(labels, rows, 1, ids, [3.0, 3.0, 3.0, 0, 0, 0, 0], label="a tie")
    assert got[0] == 10
    got, _, _ = cd.check_row_ids(labels, rows, 1, ids, None, label="no weights")
    assert got[0] == 10
    got, _, _ = cd.check_row_ids(labels, rows, 1, [-1, 11, 12, 13, 14, 15, 16], [9.0, 1.0, 1.0, 0, 0, 0, 0], label="an id -1 never wins")
    assert got[0] == 11
    got, _, _ = cd.check_row_ids(labels, rows, 1, [-1, -1, -1, 13, 14, 15, 16], None, label="only ids -1")
    assert got[0] == -1
    got, _, _ = cd.check_row_ids(labels, rows, 1, ids, [np.nan, 1.0, np.nan, 0, 0, 0, 0], label="a NaN weighs least")
    assert got[0] == 11
    got, counts, _ = cd.check_row_ids(labels, rows, 0, ids, None, label="the source side")
    assert got.tolist() == [14, -1, -1, -1, -1, -1, -1, -1, 15, -1] and counts[2] == 0          # a negative label takes no id, though a pair has it


def test_the_row_ids_are_bit_identical_on_a_rerun_and_on_a_second_stream(cd):
    pool, rows, ids, weight = cc.pair_table(1500, 3)
    labels = pool[np.random.default_rng(1).integers(0, len(pool), 3000)]
    first = cd.run_row_ids(labels, rows, 1, ids, weight)[2]
    assert cd.run_row_ids(labels, rows, 1, ids, weight)[2] == first and cd.run_row_ids(labels, rows, 1, ids, weight, stream=torch.cuda.Stream())[2] == first


# ------------------------------------------------------------------------------------------------------------------ extend_side

def _objects_of(step, other=777.0):
    """test_gpu_tracks's object rows of a gap, with a source label no segment has"""
    labels = sorted(set(step["labels"].tolist()) - {-1.0})
    rows = [tc.object_row(lab, d=(0.5 * k, 0.25, 0.0), size=(2.0 + k, 3.0, 1.5), points=10 + k, label_src=other) for k, lab in enumerate(labels)]
    return np.array(rows + [tc.object_row(999.0, label_src=other), tc.object_row(labels[0], points=0, label_src=other), tc.object_row(-1.0, label_src=other)])


def test_side_1_is_the_existing_call_bit_for_bit_on_the_chain(cd):
    import track_device as td
    state, next_id = np.full(tc.CHAIN_ROWS, -1, np.int32), 0
    for gap, step in enumerate(tc.chain(), start=1):
        objects = _objects_of(step)
        old = td.run_extend(step["labels"], state, next_id, objects, gap, 0.1 * gap)
        new = cd.check_extend_side(step["labels"], state, next_id, objects, 1, gap, 0.1 * gap, label=f"gap {gap}")
        assert new["raw"] == old["raw"]
        assert new["track_of_row"].tolist() == step["ids"].tolist() and new["obs"][:-3, 0].tolist() == step["segment_ids"][1:]
        state, next_id = new["track_of_row"], new["next_id"]


def test_side_0_reads_the_source_label_on_the_chain(cd):
    state, next_id = np.full(tc.CHAIN_ROWS, -1, np.int32), 0
    for gap, step in enumerate(tc.chain(), start=1):
        objects = cr.swapped(_objects_of(step))                 # the gap's labels in column 0, 777 in column 1
        got = cd.check_extend_side(step["labels"], state, next_id, objects, 0, gap, 0.1 * gap, label=f"gap {gap}")
        assert got["track_of_row"].tolist() == step["ids"].tolist() and got["next_id"] == step["next_id"]
        assert got["obs"][-3:, 0].tolist() == [-1, -1, -1] and got["obs"][:-3, 0].tolist() == step["segment_ids"][1:]
        wrong = cd.run_extend_side(step["labels"], state, next_id, objects, 1, gap, 0.1 * gap)
        assert (wrong["obs"][:, 0] == -1).all()                 # side 1 on the same rows finds 777 nowhere
        state, next_id = got["track_of_row"], got["next_id"]


def test_side_0_overflow_leaves_the_state_bit_for_bit(cd):
    state = (np.arange(40, dtype=np.int32) % 7) - 1
    for labels, st, nid, name in ((np.arange(40, dtype=F), state, 9, "labels"), (np.zeros(40, F), np.arange(40, dtype=np.int32), 40, "ids"),
                                  (np.arange(40, dtype=F) % 5, state, (1 << 24) - 3, "id range")):
        got = cd.check_extend_side(labels, st, nid, [tc.object_row(999.0, label_src=1.0)], 0, 2, 0.2, Lmax=16, label=name)
        assert got["num"] < 0 and got["next_id"] == nid and np.array_equal(got["track_of_row"], st), name
        assert got["counts"].tolist() == [0, 0, 0, 0, 1, 1] and got["obs"][0, 0] == -1 and len(got["segments"]) == 0


# -------------------------------------------------------------------------------------------------------------------- the paths

def test_the_hand_made_chains(cd):
    obs, step, frames, want = cc.three_step_chain()
    paths, counts, raw = cd.check_path(obs, step, frames, 2, label="adjacent steps")
    assert paths[0].tolist() == [float(v) for v in want] and paths[1].tolist() == [1.0] + [0.0] * 23 and counts.tolist() == [2, 1, 1, 0, 1]
    assert cd.run_path(obs, step, frames, 2)[2] == raw and cd.run_path(obs, step, frames, 2, stream=torch.cuda.Stream())[2] == raw
    paths, counts, _ = cd.check_path(obs, step, frames, 1, max_dv=2.0, label="exactly max_dv")
    assert paths[0, 16] == 1 and counts.tolist() == [1, 1, 1, 1, 1]
    paths, _, _ = cd.check_path([obs[0], obs[2]], [0, 2], frames, 1, label="a missing step")
    assert paths[0, 1:5].tolist() == [2, 0, 2, 1] and paths[0, 11:17].tolist() == [0, 0, 0, 1, 0, 0]
    paths, _, _ = cd.check_path(obs, [0, 0, 1], frames, 1, label="two observations in one step")
    assert paths[0, 1] == 2 and paths[0, 21:24].tolist() == [1.25, 2.0, 0.5] and paths[0, 11] == 2.0
    paths, _, _ = cd.check_path([obs[0], obs[0][:10] + [9.0, 9.0, 9.0]], [0, 0], frames, 1, label="equal points")
    assert paths[0, 21:24].tolist() == [1.0, 2.0, 0.5]
    paths, counts, _ = cd.check_path(obs, [0, 1, 3], frames, 1, label="a step outside [0, F)")
    assert paths[0, 1] == 2 and paths[0, 3] == 1
    paths, counts, _ = cd.check_path(obs, step, frames, 0, label="T = 0")
    assert paths.shape == (0, 24) and counts.tolist() == [0] * 5
    paths, counts, _ = cd.check_path(np.zeros((0, 13)), [], np.zeros((0, 12)), 300, label="M = 0")
    assert (paths[:, 0] == np.arange(300)).all() and not paths[:, 1:].any() and counts.tolist() == [300, 0, 0, 0, 0]


def test_300_seeded_tables_with_rotations(cd):
    """every table of its own would be 300 launches; they are stacked into calls of 30 tables each -- the tracks of table j
    renumbered to 6 j .. 6 j + 5, the files of every table the same five, so the steps stay non-decreasing per track"""
    for call in range(10):
        obs, step, T = [], [], 0
        tables = [cc.random_path_table(1000 * call + j) for j in range(30)]
        frames = tables[0][2]
        for j, (o, s, _, t) in enumerate(tables):
            o = o.copy()
            o[:, 0] = np.where((o[:, 0] >= 0) & (o[:, 0] < t), o[:, 0] + T, -1.0)
            obs.append(o), step.append(s)
            T += t
        paths, counts, _ = cd.check_path(np.concatenate(obs), np.concatenate(step), frames, T, label=f"call {call}")
        assert counts[0] == T == 180 and counts[1] > 100 and counts[2] > 20 and 0 < counts[3] <= counts[2]


# ------------------------------------------------------------------------------------------------------------ the Python layer

def test_the_device_wrappers_give_what_the_raw_calls_give(cd):
    from icp_flow_amd import utils_tracks
    up = cd.upload
    pose = cc.POSES["yaw30"]
    prev, prev_id, nxt = cc.views(2049, 513, 9, pose)
    ids, counts = utils_tracks.rows_carry_device(up(prev, F), up(prev_id, np.int32), pose, up(nxt, F), cc.RADIUS, 0.25)
    want = cr.rows_carry(prev, prev_id, pose, nxt, cc.RADIUS, 0.25)
    assert np.array_equal(ids.cpu().numpy(), want["id"]) and np.array_equal(counts.cpu().numpy(), want["counts"])
    pool, rows, pid, weight = cc.pair_table(300, 8)
    labels = pool[np.random.default_rng(2).integers(0, len(pool), 1500)]
    objects = np.zeros((300, 24))
    objects[:, 22] = weight
    got, counts = utils_tracks.pair_row_ids_device(up(labels, F), up(rows, F), 1, up(pid, np.int32), up(objects, np.float64)[:, 22])
    want_ids, want_counts = cr.pair_row_ids(labels, rows, 1, pid, weight)
    assert np.array_equal(got.cpu().numpy(), want_ids) and np.array_equal(counts.cpu().numpy(), want_counts)
    # a state seeded with carried ids and a running counter, taken by reference; side 0
    step = tc.chain()[1]
    seed_ids, counter = up(tc.chain()[0]["ids"], np.int32), up(np.array([6], np.int32), np.int32)
    state = utils_tracks.TrackState(tc.CHAIN_ROWS, cd.DEV, Lmax=16, track_of_row=seed_ids, next_id=counter, bound=6)
    objects = cr.swapped(_objects_of(step))
    state.extend(up(step["labels"], F), up(objects, np.float64), 0, 0.1, side=0)
    assert state.track_of_row is seed_ids and seed_ids.cpu().numpy().tolist() == step["ids"].tolist() and int(counter) == step["next_id"] == 7
    assert state.obs[0][:-3, 0].cpu().numpy().tolist() == step["segment_ids"][1:] and state.bound == 6 + 16

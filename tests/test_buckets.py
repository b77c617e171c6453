"""CPU-only: the host side of the bucket-normalised EPE (Argoverse 2, 2024 challenge).  icpflow_seq_bucket_table is bound and
refuses what it must with status codes and messages (no launch: there is no GPU here), its workspace size is the documented
formula; the edges and the challenge's groups; utils_eval.bucketed_epe on a table counted by hand; BucketTable's arithmetic;
the numpy restatement the GPU tests hold the kernel against (tests/bucket_restatement.py) counts, over all its cells, what the
REFERENCE recorded as `overall` for the demo sample of the g15 fixtures; and the gather-and-replay of a sharded run (gloo,
1 / 2 / 3 ranks) bit for bit against a single process."""
import ctypes
import math
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import argo_restatement as ar         # noqa: E402
import bucket_restatement as br       # noqa: E402
import class_restatement as cr        # noqa: E402
import seqeval_restatement as sr      # noqa: E402

EDGES50 = tuple(np.linspace(0.0, 2.0, 51)[1:])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def _call(m=10, F=2, crop=2, G=33, S=51, speed=EDGES50, class_lo=-1.0, ws=1 << 30, null=None):
    from icp_flow_amd import _lib
    one = ctypes.c_void_p(16)
    sp = np.asarray(speed, np.float64)
    ptrs = {k: one for k in ("pts", "tim", "cls", "gt", "pred", "table", "info", "ws")}
    ptrs["speed"] = sp.ctypes.data_as(ctypes.c_void_p)
    if null:
        ptrs[null] = None
    rc = _lib._L.icpflow_seq_bucket_table(ptrs["pts"], ptrs["tim"], ptrs["cls"], ptrs["gt"], ptrs["pred"], m, F, crop, 35.0, 35.0, 0.3, class_lo,
                                          G, ptrs["speed"], S, ptrs["table"], ptrs["info"], ptrs["ws"], ctypes.c_size_t(ws), None)
    return rc, _lib._L.icpflow_last_error().decode()


def _formula(m, G, S):
    """align256(grid(m) * (G * S * 3 + 2) * 8), grid(m) = ceil(m / 2048) clamped to [1, 256]"""
    grid = min(max(-(-m // 2048), 1), 256)
    return -(-grid * (G * S * 3 + 2) * 8 // 256) * 256


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib
    assert "icpflow_seq_bucket_table" in _lib.SIGNATURES and "icpflow_seq_bucket_table_workspace_bytes" in _lib.SIGNATURES
    assert (_lib.BUCKET_MAX_ROWS, _lib.BUCKET_MAX_BUCKETS) == (64, 64)
    with open(os.path.join(br.REPO, "include", "icpflow_hip.h")) as f:
        hdr = f.read()
    assert "#define ICPFLOW_BUCKET_MAX_ROWS 64" in hdr and "#define ICPFLOW_BUCKET_MAX_BUCKETS 64" in hdr
    size = _lib._L.icpflow_seq_bucket_table_workspace_bytes
    for m in (0, 1, 2048, 2049, 126598, 524288, 524288 + 777, 1 << 30, (1 << 31) - 1):
        for G, S in ((33, 51), (2, 1), (64, 64), (33, 3)):
            assert size(m, G, S) == _formula(m, G, S), (m, G, S)
    assert size(126598, 33, 51) == -(-62 * 5051 * 8 // 256) * 256 and size(0, 2, 1) == 256
    for bad in ((-1, 33, 51), (10, 1, 51), (10, 33, 0), (10, 65, 2), (10, 2, 65), (10, 0, 0)):
        assert size(*bad) == 0, bad


def test_every_refusal_is_a_status_code_with_a_message():
    assert _call(m=-1) == (-1, "icpflow_seq_bucket_table: m < 0")
    rc, msg = _call(F=0)
    assert rc == -1 and "F must be >= 1" in msg
    rc, msg = _call(crop=3)
    assert rc == -1 and "crop must be" in msg
    rc, msg = _call(G=1)
    assert rc == -1 and "G must be >= 2" in msg
    rc, msg = _call(S=0)
    assert rc == -1 and "S must be >= 1" in msg
    for kw in (dict(G=65, S=2, speed=(0.1,)), dict(G=2, S=65, speed=tuple(range(64)))):
        rc, msg = _call(**kw)
        assert rc == -3 and "at most 64 rows and 64 buckets" in msg, (kw, msg)
    assert _call(G=64, S=64, speed=tuple(range(63)), ws=16)[0] == -2            # the limits themselves pass the limit check
    for null in ("pts", "tim", "cls", "gt", "pred", "table", "info", "speed"):
        rc, msg = _call(null=null)
        assert (rc, msg) == (-1, "icpflow_seq_bucket_table: null pointer"), null
    assert _call(m=0, null="pts", ws=16)[0] == -2                               # no rows: the row arrays may be null
    assert _call(S=1, speed=(), null="speed", ws=16)[0] == -2                   # no edges: the list may be null
    for bad in ((0.2, 0.05), (0.05, 0.05), (0.05, float("inf")), (float("nan"), 0.1), (float("-inf"), 0.1)):
        rc, msg = _call(S=3, speed=bad)
        assert rc == -1 and "finite and strictly ascending" in msg, bad
    for lo in (0.5, float("nan"), float("inf")):
        rc, msg = _call(class_lo=lo)
        assert rc == -1 and "class_lo" in msg
    rc, msg = _call(ws=16)
    assert rc == -2 and f"icpflow_seq_bucket_table_workspace_bytes says {_formula(10, 33, 51)}" in msg
    rc, msg = _call(null="ws")
    assert rc == -2 and "workspace" in msg


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_eval
    s, pred = cr.fixture_sample("g15_argo_f64")
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.bucket_table(ar.setting_args("argo"), data, torch.from_numpy(pred))


def test_bucketed_epe_flag_needs_the_argoverse_protocol(tmp_path):
    from icp_flow_amd import frame_pairs
    for argv in (["--bucketed-epe"], ["--bucketed-epe", "--protocol", "reference"], ["--bucketed-epe", "--dataset", "argo"],
                 ["--bucketed-epe", "--protocol", "reference", "--dataset", "pca"]):
        with pytest.raises(SystemExit, match="--bucketed-epe goes with --protocol reference --dataset argo"):
            frame_pairs.main([str(tmp_path)] + argv)


# ---- the constants --------------------------------------------------------------------------------------------------------
def test_edges_are_numpys_linspace_bit_for_bit():
    from icp_flow_amd import utils_eval
    got = np.asarray(utils_eval.ARGO_BUCKET_EDGES, np.float64)
    want = np.linspace(0, 2, 51)[1:]
    assert got.shape == (50,) and got.tobytes() == want.tobytes() == br.EDGES.tobytes()
    assert (np.diff(got) > 0).all() and got[0] == 0.04 and got[-1] == 2.0


def test_every_group_name_resolves_and_no_row_is_in_two_groups():
    from icp_flow_amd import utils_eval
    names = utils_eval.ARGO_ROW_NAMES
    assert list(names) == br.row_names()
    groups = utils_eval.ARGO_CHALLENGE_GROUPS
    assert list(groups) == ["BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU"]
    assert {g: list(rows) for g, rows in groups.items()} == br.groups()
    for g, rows in groups.items():
        assert [names[r] for r in rows] == sorted(br.GROUP_NAMES[g], key=names.index) and len(rows) == len(br.GROUP_NAMES[g])
    used = [r for rows in groups.values() for r in rows]
    assert len(used) == len(set(used)) == 30
    assert [names[r] for r in sorted(set(range(33)) - set(used))] == br.UNGROUPED
    assert names[groups["CAR"][0]] == "REGULAR_VEHICLE" and 0 in groups["BACKGROUND"]


# ---- the metric on a table counted by hand -----------------------------------------------------------------------------------
def _hand_table():
    """(33, 51).  REGULAR_VEHICLE (row 20): bucket 0 with 4 rows, sum e 0.2; bucket 3 with 2 rows, sum e 0.03, sum |gt| 0.3;
    bucket 50 with 1 row, e 1.5, |gt| 3.0.  TRUCK (row 26) and BUS (row 8), both OTHER_VEHICLES: bucket 3 with sum e 0.1 + 0.2,
    sum |gt| 0.25 + 0.5.  PEDESTRIAN (row 18): static rows only, 5 rows, sum e 0.5.  WHEELED_VRU: nothing.  DOG (row 11):
    bucket 0 with 1 row, e 9; bucket 1 with 1 row, e 8, |gt| 0.05.  BACKGROUND: UNLABELLED (row 0) 10 static rows, sum e 0.1."""
    from icp_flow_amd import utils_eval
    t = utils_eval.BucketTable.zeros(33, 51)
    for row, b, n, e, s in ((20, 0, 4, 0.2, 0.01), (20, 3, 2, 0.03, 0.3), (20, 50, 1, 1.5, 3.0), (26, 3, 1, 0.1, 0.25), (8, 3, 2, 0.2, 0.5),
                            (18, 0, 5, 0.5, 0.02), (11, 0, 1, 9.0, 0.0), (11, 1, 1, 8.0, 0.05), (0, 0, 10, 0.1, 0.0)):
        t.counts[row, b], t.esum[row, b], t.ssum[row, b] = n, e, s
    return t


def test_bucketed_epe_on_a_hand_counted_table():
    from icp_flow_amd import utils_eval
    res = utils_eval.bucketed_epe(_hand_table())
    assert list(res) == ["BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU", "OTHER", "mean_static", "mean_dynamic"]
    # two dynamic buckets: the ratio per bucket, then their plain mean (NOT sum e / sum |gt| over the buckets: 1.53 / 3.3)
    car = res["CAR"]
    assert car == dict(static=0.2 / 4, dynamic=(0.03 / 0.3 + 1.5 / 3.0) / 2, n_static=4, n_dynamic=3, buckets_used=2)
    assert car["dynamic"] != (0.03 + 1.5) / (0.3 + 3.0)
    # two rows of a group in one bucket: added in ascending row order (BUS before TRUCK), then the ratio
    ov = res["OTHER_VEHICLES"]
    assert ov["dynamic"] == (0.2 + 0.1) / (0.5 + 0.25) and math.isnan(ov["static"]) and (ov["n_static"], ov["n_dynamic"], ov["buckets_used"]) == (0, 3, 1)
    # static rows only: the dynamic value is NaN and the mean skips it
    ped = res["PEDESTRIAN"]
    assert ped["static"] == 0.5 / 5 and math.isnan(ped["dynamic"]) and ped["buckets_used"] == 0 and ped["n_dynamic"] == 0
    # an empty class
    vru = res["WHEELED_VRU"]
    assert math.isnan(vru["static"]) and math.isnan(vru["dynamic"]) and (vru["n_static"], vru["n_dynamic"], vru["buckets_used"]) == (0, 0, 0)
    assert res["BACKGROUND"]["static"] == 0.1 / 10 and math.isnan(res["BACKGROUND"]["dynamic"])
    # rows in no group are reported and enter neither mean
    assert res["OTHER"] == dict(static=9.0, dynamic=8.0 / 0.05, n_static=1, n_dynamic=1, buckets_used=1)
    assert res["mean_static"] == (0.1 / 10 + 0.2 / 4 + 0.5 / 5) / 3 and res["mean_dynamic"] == (car["dynamic"] + ov["dynamic"]) / 2
    empty = utils_eval.bucketed_epe(utils_eval.BucketTable.zeros(33, 51))
    assert math.isnan(empty["mean_static"]) and math.isnan(empty["mean_dynamic"])
    lines = utils_eval.format_bucketed_epe(res).split("\n")
    assert len(lines) == 1 + 6 + 1 and lines[2].startswith("             CAR, static EPE: 0.050000 (n 4), dynamic normalised EPE: 0.300000 (n 3, 2 buckets)")
    assert lines[-1] == f"mean static EPE: {res['mean_static']:.6f}, mean dynamic normalised EPE: {res['mean_dynamic']:.6f}"


def test_add_meta_and_words_are_exact():
    from icp_flow_amd import utils_eval
    t = _hand_table()
    t.kept0 = 7
    again = utils_eval.BucketTable.from_words(t.words(), 33, 51, kept0=7)
    assert np.array_equal(again.counts, t.counts) and again.esum.tobytes() == t.esum.tobytes() and again.ssum.tobytes() == t.ssum.tobytes()
    assert t.words().shape == (33 * 51 * 3,) and t.words().reshape(33, 51, 3)[20, 3].tolist() == [2, np.float64(0.03).view(np.int64), np.float64(0.3).view(np.int64)]
    twice = utils_eval.BucketTable.zeros(33, 51).add(t).add(t)
    assert np.array_equal(twice.counts, 2 * t.counts) and np.array_equal(twice.esum, t.esum + t.esum) and twice.kept0 == 14
    with pytest.raises(ValueError):
        t.add(utils_eval.BucketTable.zeros(33, 3))
    meta = t.meta(utils_eval.ARGO_CHALLENGE_GROUPS)
    assert meta.names == ("BACKGROUND", "CAR", "OTHER_VEHICLES", "PEDESTRIAN", "WHEELED_VRU", "OTHER") and meta.counts.shape == (6, 51)
    assert int(meta.counts.sum()) == int(t.counts.sum()) == 27 and meta.kept0 == 7
    for k, rows in enumerate(list(utils_eval.ARGO_CHALLENGE_GROUPS.values()) + [(2, 11, 32)]):
        assert np.array_equal(meta.counts[k], t.counts[list(rows)].sum(axis=0))
        acc = np.zeros(51)
        for r in sorted(rows):
            acc = acc + t.esum[r]
        assert meta.esum[k].tobytes() == acc.tobytes()
    with pytest.raises(ValueError):
        t.meta({"A": (1, 2), "B": (2,)})


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_restatement_on_a_scene_counted_by_hand():
    """Eight rows, F = 3, crop |x| < 32, |y| < 32, z > 0.3, zero predictions, so e = |gt|."""
    args = SimpleNamespace(num_frames=3, eval_ground=False, range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
    raw = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [40, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float64)
    t = np.array([0, 1, 2, 1, 1, 3, 2, 1])
    cls = np.array([np.nan, -1, 19, 19, 3.5, 19, 19, 30])
    gt = np.array([[0, 0, 0], [0.03, 0, 0], [0.04, 0, 0], [1, 0, 0], [0, 0, 0.5], [1, 0, 0], [0, 0, 2.0], [np.nan, 0, 0]], np.float64)
    c = br.table(args, dict(raw_points=raw, time_indice=t, scene_flow=gt), np.zeros((8, 3), np.float32), cls)
    assert (c.kept0, c.outside) == (1, 1) and int(c.counts.sum()) == 5
    # row 1: -1 -> row 0, 0.03 -> bucket 0.  row 2: 19 -> row 20 (REGULAR_VEHICLE), 0.04 -> bucket 1 (lower edge inclusive).  row 3: cropped.
    # row 4: 3.5 -> row 32, 0.5 -> bucket 12 (twelve edges 0.04 .. 0.48 are <= 0.5).  row 5: time index outside.  row 6: 2.0 -> the
    # last bucket.  row 7: a NaN speed -> bucket 0, in row 31.
    assert c.counts[0, 0] == 1 and c.counts[20, 1] == 1 and c.counts[32, 12] == 1 and c.counts[20, 50] == 1 and c.counts[31, 0] == 1
    assert c.e[20][1] == [0.04] and c.speed[32][12] == [0.5] and c.e[20][50] == [2.0]
    m = br.metric(c)
    assert m["CAR"]["dynamic"] == (0.04 / 0.04 + 2.0 / 2.0) / 2 and m["CAR"]["buckets_used"] == 2 and m["BACKGROUND"]["static"] == 0.03
    assert m["OTHER"]["n_dynamic"] == 1 and math.isnan(m["WHEELED_VRU"]["static"])


@pytest.mark.parametrize("setting", list(ar.SETTINGS))
def test_restatement_total_equals_the_references_overall_count(setting):
    """The demo sample of G15 under each of its three settings: the rows in all cells are the rows the REFERENCE recorded
    under `overall`, and the product's BucketTable / bucketed_epe on the restatement's sequential sums agree with the
    restatement's metric within the summation bound."""
    from icp_flow_amd import utils_eval
    s, pred = cr.fixture_sample(ar.DEMO)
    g = ar.load(ar.DEMO)
    names = [str(n) for n in g["meter_names"]]
    c = br.table(ar.setting_args(setting), s, pred, s["classes"])
    want = int(g[setting + "_num"][names.index("overall_1")])
    assert c.outside == 0 and int(c.counts.sum()) == want and want > 10000
    print(f"{setting}: {want} rows in {int((c.counts > 0).sum())} cells")
    t = utils_eval.BucketTable(c.counts, c.sequential("e"), c.sequential("speed"), c.kept0)
    got, ref = utils_eval.bucketed_epe(t), br.metric(c)
    for name in list(utils_eval.ARGO_CHALLENGE_GROUPS) + ["OTHER"]:
        for key in ("n_static", "n_dynamic", "buckets_used"):
            assert got[name][key] == ref[name][key], (name, key)
        for key in ("static", "dynamic"):
            a, b = got[name][key], ref[name][key]
            assert math.isnan(a) == math.isnan(b) and (math.isnan(a) or abs(a - b) <= br.metric_tolerance(want) * abs(b)), (name, key, a, b)
    for key in ("mean_static", "mean_dynamic"):
        assert abs(got[key] - ref[key]) <= br.metric_tolerance(want) * abs(ref[key]), key


# ---- ranks ----------------------------------------------------------------------------------------------------------------
CLASS_SHAPE, BUCKET_SHAPE = (33, 3, 3), (33, 51)


def _five_records(with_classes):
    """Five files' records: tables of the seqeval restatement on a g13 sample (F = 3) under five predictions, bucket tables (and
    class tables) of the restatements on a g15 sample under five predictions -- two of them empty."""
    from icp_flow_amd import frame_pairs, utils_eval
    g = sr.load("g13_seqeval_f3_f64")
    args = sr.crop_args(g, 0)
    data = sr.sample(g)
    s, pred_c = cr.fixture_sample("g15_argo_f64")
    rng = np.random.default_rng(17)
    records = []
    for k in range(5):
        pred = (g["pred_flow"] + rng.normal(scale=0.05 * k, size=g["pred_flow"].shape)).astype(np.float32)
        table, esum, kept0 = sr.table_numpy(args, data, pred)
        table[:, :, 1] = esum.view(np.int64)
        if k in (1, 4):
            classes, buckets = utils_eval.ClassTable.zeros(*CLASS_SHAPE), utils_eval.BucketTable.zeros(*BUCKET_SHAPE)
        else:
            p = (pred_c + rng.normal(scale=0.02 * k, size=pred_c.shape)).astype(np.float32)
            c = cr.table(ar.setting_args("argo"), s, p, s["classes"])
            classes = utils_eval.ClassTable(c.counts, c.sequential("e"), c.sequential("speed"), c.kept0)
            b = br.table(ar.setting_args("argo"), s, p, s["classes"])
            buckets = utils_eval.BucketTable(b.counts, b.sequential("e"), b.sequential("speed"), b.kept0)
        records.append(frame_pairs.sequence_record(k, 3, table, kept0, 2, (1000.0 + k, 100.0 + k, 0.0), classes if with_classes else None,
                                                   buckets=buckets))
    return args, np.stack(records)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merge_worker(rank, world, port, records_path, out_dir, with_classes):
    import torch.distributed as dist
    from icp_flow_amd import frame_pairs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    with np.load(records_path) as z:
        records, args = z["records"], SimpleNamespace(num_frames=int(z["num_frames"]))
    mine = [records[k] for k in range(len(records))][rank::world]
    metrics, classes, heads, buckets = frame_pairs.merge_sequence_records(args, mine, len(records), rank, world,
                                                                          class_shape=CLASS_SHAPE if with_classes else None,
                                                                          bucket_shape=BUCKET_SHAPE)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), heads=heads, bucket_words=buckets.words(), bucket_kept0=np.array(buckets.kept0),
             class_words=classes.words() if with_classes else np.zeros(0, np.int64), overall_0=np.array([metrics["overall_0"].epe_sum, metrics["overall_0"].num]))
    dist.destroy_process_group()


@pytest.mark.parametrize("with_classes", [False, True], ids=["buckets", "classes_and_buckets"])
def test_sharded_replay_is_bit_identical_to_a_single_process(tmp_path, with_classes):
    """merge_sequence_records with bucket_shape under gloo on 1, 2 and 3 ranks (shares 5; 3 + 2; 2 + 2 + 1): every rank's
    bucket table (and class table, when the records carry both) equals the plain replay in file order bit for bit."""
    import torch.multiprocessing as mp
    from icp_flow_amd import frame_pairs, utils_eval
    args, records = _five_records(with_classes)
    H, cw = frame_pairs.RECORD_HEAD, (33 * 3 * 5 if with_classes else 0)
    assert records.shape == (5, H + 108 + cw + 33 * 51 * 3)
    want_m, want_c, want_b = utils_eval.new_metric_table(3), utils_eval.ClassTable.zeros(*CLASS_SHAPE), utils_eval.BucketTable.zeros(*BUCKET_SHAPE)
    for r in records:
        table = r[H:H + 108].reshape(3, 6, 6).copy()
        utils_eval.update_meters(args, want_m, table, np.ascontiguousarray(table[:, :, 1]).view(np.float64), int(r[1]))
        if with_classes:
            want_c.add(utils_eval.ClassTable.from_words(r[H + 108:H + 108 + cw], *CLASS_SHAPE, kept0=int(r[1])))
        want_b.add(utils_eval.BucketTable.from_words(r[H + 108 + cw:], *BUCKET_SHAPE, kept0=int(r[1])))
    assert int(want_b.counts.sum()) > 0 and int((want_b.counts > 0).sum()) > 20
    records_path = str(tmp_path / "records.npz")
    np.savez(records_path, records=records, num_frames=np.array(3))
    for world in (1, 2, 3):
        out_dir = str(tmp_path / f"world{world}")
        os.makedirs(out_dir)
        mp.spawn(_merge_worker, args=(world, _free_port(), records_path, out_dir, with_classes), nprocs=world, join=True)
        for rank in range(world):
            with np.load(os.path.join(out_dir, f"rank{rank}.npz")) as z:
                assert z["bucket_words"].tobytes() == want_b.words().tobytes() and int(z["bucket_kept0"]) == want_b.kept0, (world, rank)
                if with_classes:
                    assert z["class_words"].tobytes() == want_c.words().tobytes(), (world, rank)
                assert z["overall_0"].tobytes() == np.array([want_m["overall_0"].epe_sum, want_m["overall_0"].num]).tobytes()
                assert np.array_equal(z["heads"], records[:, :H])
    # without bucket_shape the call is what it was: three results, and a record with a bucket table is of the wrong length
    with pytest.raises(ValueError):
        frame_pairs.merge_sequence_records(args, list(records), 5, class_shape=CLASS_SHAPE if with_classes else None)
    with pytest.raises(RuntimeError, match="do not cover"):
        frame_pairs.merge_sequence_records(args, list(records[1:]), 5, class_shape=CLASS_SHAPE if with_classes else None, bucket_shape=BUCKET_SHAPE)
    with pytest.raises(TypeError):
        frame_pairs.merge_sequence_records(args, list(records), 5, 0, 1, None, None, None, BUCKET_SHAPE)     # keyword-only

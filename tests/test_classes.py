"""CPU-only: the per-class table's host side.  icpflow_seq_class_table is bound and refuses what it must with status codes and
messages (no launch: there is no GPU here); the product's Argoverse 2 names and groups equal what the reference's loader
carries (tests/golden/g16_argo_classes.json, tools/gen_golden_argo_classes.py); the numpy restatement the GPU tests hold the
kernel against (tests/class_restatement.py) is checked on a scene counted by hand and -- its marginals -- against the
REFERENCE's recorded meters of the g15 fixtures; ClassTable's arithmetic, the printed lines, the save path rule, the metrics
file and the gather-and-replay of a sharded run (gloo, 1 / 2 / 3 ranks) bit for bit against a single process."""
import ctypes
import json
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
import class_restatement as cr        # noqa: E402
import seqeval_restatement as sr      # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ar.SYNTHETIC + (ar.DEMO,)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def _call(m=10, F=2, crop=2, G=33, S=3, E=3, speed=(0.05, 0.2), error=(0.05, 0.1), class_lo=-1.0, ws=1 << 30, null=None):
    from icp_flow_amd import _lib
    one = ctypes.c_void_p(16)
    sp, er = np.asarray(speed, np.float64), np.asarray(error, np.float64)
    ptrs = {k: one for k in ("pts", "tim", "cls", "gt", "pred", "table", "info", "ws")}
    ptrs["speed"], ptrs["error"] = sp.ctypes.data_as(ctypes.c_void_p), er.ctypes.data_as(ctypes.c_void_p)
    if null:
        ptrs[null] = None
    rc = _lib._L.icpflow_seq_class_table(ptrs["pts"], ptrs["tim"], ptrs["cls"], ptrs["gt"], ptrs["pred"], m, F, crop, 32.0, 32.0, 0.3, class_lo,
                                         G, ptrs["speed"], S, ptrs["error"], E, ptrs["table"], ptrs["info"], ptrs["ws"], ctypes.c_size_t(ws), None)
    return rc, _lib._L.icpflow_last_error().decode()


def test_exports_are_bound_and_sized():
    from icp_flow_amd import _lib
    L = _lib._L
    assert "icpflow_seq_class_table" in _lib.SIGNATURES and "icpflow_seq_class_table_workspace_bytes" in _lib.SIGNATURES
    assert (_lib.CLASS_MAX_ROWS, _lib.CLASS_MAX_BUCKETS, _lib.CLASS_MAX_WORDS) == (64, 8, 1024)
    size = L.icpflow_seq_class_table_workspace_bytes
    # a workgroup per 2048 rows, 256 at most; G * S * (E + 2) + 2 words each; 256-byte multiples
    for m, grid in ((0, 1), (1, 1), (2048, 1), (2049, 2), (126598, 62), (524288 + 777, 256), (1 << 30, 256)):
        assert size(m, 33, 3, 3) == -(-grid * (495 + 2) * 8 // 256) * 256, m
    assert size(100, 64, 2, 6) == -(-(1024 + 2) * 8 // 256) * 256 and size(100, 2, 1, 1) == 256
    for bad in ((-1, 33, 3, 3), (10, 1, 3, 3), (10, 33, 0, 3), (10, 33, 3, 0), (10, 65, 1, 1), (10, 2, 9, 1), (10, 2, 1, 9), (10, 64, 2, 7)):
        assert size(*bad) == 0, bad


def test_every_refusal_is_a_status_code_with_a_message():
    assert _call(m=-1) == (-1, "icpflow_seq_class_table: m < 0")
    rc, msg = _call(F=0)
    assert rc == -1 and "F must be >= 1" in msg
    rc, msg = _call(crop=3)
    assert rc == -1 and "crop must be" in msg
    rc, msg = _call(G=1)
    assert rc == -1 and "G must be >= 2" in msg
    for kw in (dict(S=0), dict(E=0)):
        rc, msg = _call(**kw)
        assert rc == -1 and "S and E must be >= 1" in msg
    # the limits, each by itself and the product: 64 x 2 x (6 + 2) = 1024 words pass, 64 x 2 x (7 + 2) do not
    for kw in (dict(G=65, S=1, E=1, speed=(), error=()), dict(G=2, S=9, E=1, speed=tuple(range(8)), error=()),
               dict(G=2, S=1, E=9, speed=(), error=tuple(range(8))), dict(G=64, S=2, E=7, speed=(0.1,), error=tuple(range(6)))):
        rc, msg = _call(**kw)
        assert rc == -3 and "1024 words" in msg, (kw, msg)
    assert _call(G=64, S=2, E=6, speed=(0.1,), error=tuple(range(5)), ws=16)[0] == -2
    for null in ("pts", "tim", "cls", "gt", "pred", "table", "info", "speed", "error"):
        rc, msg = _call(null=null)
        assert rc == -1 and "null pointer" in msg, null
    for kw in (dict(speed=(0.2, 0.05)), dict(speed=(0.05, 0.05)), dict(error=(0.1, 0.05)), dict(speed=(0.05, float("inf"))),
               dict(error=(float("nan"), 0.1)), dict(speed=(float("-inf"), 0.1))):
        rc, msg = _call(**kw)
        assert rc == -1 and "finite and strictly ascending" in msg, kw
    for lo in (0.5, float("nan"), float("inf")):
        rc, msg = _call(class_lo=lo)
        assert rc == -1 and "class_lo" in msg
    rc, msg = _call(ws=16)
    assert rc == -2 and "icpflow_seq_class_table_workspace_bytes says 4096" in msg
    rc, msg = _call(null="ws")
    assert rc == -2 and "workspace" in msg


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_eval
    s, pred = cr.fixture_sample("g15_argo_f64")
    data = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()}
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_eval.class_table(ar.setting_args("argo"), data, torch.from_numpy(pred))


def test_class_table_flag_needs_the_argoverse_protocol(tmp_path):
    from icp_flow_amd import frame_pairs
    for argv in (["--class-table", "meta"], ["--class-table", "fine", "--protocol", "reference"], ["--class-table", "meta", "--dataset", "argo"]):
        with pytest.raises(SystemExit, match="--class-table goes with --protocol reference --dataset argo"):
            frame_pairs.main([str(tmp_path)] + argv)
    with pytest.raises(SystemExit, match="go with --protocol reference"):
        frame_pairs.main([str(tmp_path), "--save-flows"])


# ---- the product's constants ------------------------------------------------------------------------------------------
def test_constants_equal_what_the_reference_carries():
    from icp_flow_amd import utils_eval, utils_loading
    with open(os.path.join(REPO, "tests", "golden", "g16_argo_classes.json")) as f:
        g = json.load(f)
    names = utils_eval.ARGO_CATEGORY_NAMES
    assert list(names) == g["names_by_position"] and len(names) == 31 and g["first_id"] == -1
    assert list(names[1:]) == sorted(names[1:])                       # the public taxonomy, alphabetical, behind the first name
    assert utils_eval.ARGO_ROW_NAMES == ("UNLABELLED",) + names + ("OTHER",) and len(utils_eval.ARGO_ROW_NAMES) == utils_eval.ARGO_CLASS_ROWS == 33
    assert utils_eval.ARGO_CLASS_LO == -1
    row = lambda name: names.index(name) + 1                           # noqa: E731  (file value = position, row = file value + 1)
    assert list(utils_eval.ARGO_META_GROUPS) == list(g["meta"]) == ["BACKGROUND", "PEDESTRIAN", "SMALL_MOVERS", "LARGE_MOVERS"]
    for group, members in g["meta"].items():
        want = sorted(row(n) for n in members) if group != "BACKGROUND" else sorted([0] + [row(n) for n in members])
        assert list(utils_eval.ARGO_META_GROUPS[group]) == want, group
    # the background indexes: positions of the BACKGROUND names, compared with the file's values
    assert list(utils_loading.ARGO_BACKGROUND_IDXES) == g["background_idxes"] == [names.index(n) for n in g["meta"]["BACKGROUND"]]
    assert [r - 1 for r in utils_eval.ARGO_META_GROUPS["BACKGROUND"]] == [-1] + list(utils_loading.ARGO_BACKGROUND_IDXES)
    assert cr.BACKGROUND_ROWS == utils_eval.ARGO_META_GROUPS["BACKGROUND"]
    # rows in no group: file value 0, ANIMAL, DOG and the last row
    used = {r for rows in utils_eval.ARGO_META_GROUPS.values() for r in rows}
    assert sorted(set(range(33)) - used) == [1, row("ANIMAL"), row("DOG"), 32] and len(used) == sum(len(v) for v in utils_eval.ARGO_META_GROUPS.values())
    # the splits: [0, 0.5, 2, inf] m/s at 10 Hz, [0, 0.05, 0.1, inf] m
    assert g["speed_splits_m_per_s"][0] == 0 and g["speed_splits_m_per_s"][-1] == "inf" and g["error_splits_m"][0] == 0 and g["error_splits_m"][-1] == "inf"
    assert utils_eval.ARGO_SPEED_EDGES == tuple(x * 0.1 for x in g["speed_splits_m_per_s"][1:-1]) == cr.SPEED_EDGES
    assert utils_eval.ARGO_ERROR_EDGES == tuple(g["error_splits_m"][1:-1]) == cr.ERROR_EDGES
    assert utils_eval.ARGO_SPEED_EDGES[0] == utils_loading.ARGO_DYNAMIC_THRESHOLD


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_restatement_on_a_scene_counted_by_hand():
    """Nine rows, F = 3, crop |x| < 32, |y| < 32, z > 0.3; predictions zero except where noted, so e = |gt|."""
    args = SimpleNamespace(num_frames=3, eval_ground=False, range_x=32.0, range_y=32.0, range_z=0.0, ground_slack=0.3)
    raw = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [40, 0, 1], [0, 0, 0.2], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float64)
    t = np.array([0, 1, 2, 1, 1, 1, 3, -1, 2])
    cls = np.array([np.nan, -1, 5, 5, 5, 3.5, 5, 5, 30])
    gt = np.array([[0, 0, 0], [0.03, 0, 0], [0.05, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0.3, 0.4], [1, 0, 0], [1, 0, 0], [0, 0, 0.2]], np.float64)
    pred = np.zeros((9, 3), np.float32)
    pred[8] = (0, 0, 0.125)                                           # e = 0.2 - 0.125 (one subtraction)
    c = cr.table(args, dict(raw_points=raw, time_indice=t, scene_flow=gt), pred, cls)
    assert (c.kept0, c.outside) == (1, 2) and int(c.counts.sum()) == 4
    # row 1: class -1 -> row 0, speed 0.03 -> bucket 0, e 0.03 -> split 0.  row 2: class 5 -> row 6, speed 0.05 -> bucket 1 (lower
    # edge inclusive), e 0.05 -> split 1.  rows 3, 4: cropped.  row 5: class 3.5 -> row 32, speed 0.5 -> bucket 2, e 0.5 -> split 2.
    # row 8: class 30 -> row 31, speed 0.2 -> bucket 2, e 0.075 -> split 1.
    assert c.counts[0, 0, 0] == 1 and c.counts[6, 1, 1] == 1 and c.counts[32, 2, 2] == 1 and c.counts[31, 2, 1] == 1
    assert c.e[0][0] == [0.03] and c.e[6][1] == [0.05] and c.e[32][2] == [0.5] and c.e[31][2] == [0.2 - 0.125] and c.speed[31][2] == [0.2]
    assert c.sums("e")[32, 2] == 0.5 and c.sums("speed")[6, 1] == 0.05 and c.bounds("e").max() == 0.0
    # (2, 1, 1): one class row for the value 5 and the row of everything else, no edges
    c = cr.table(args, dict(raw_points=raw, time_indice=t, scene_flow=gt), pred, cls, (), (), 5, 2)
    assert c.counts.tolist() == [[[1]], [[3]]] and c.e[1][0] == [0.03, 0.5, 0.2 - 0.125]


def _stored_rows(name):
    """frame 1 of a fixture from its stored values -> (|gt| float64, e float64)"""
    s, pred = cr.fixture_sample(name)
    rows = s["time_indice"] == 1
    with np.errstate(all="ignore"):
        e, _ = sr.errors(s["scene_flow"][rows], pred[rows])
    return cr.row_speed(s["scene_flow"][rows]), e


def test_margin_conditions_hold_on_the_fixtures():
    """No |gt| within 1e-6 (relative) of a speed edge, no e within 1e-9 of an error edge: the lower-inclusive buckets cannot
    differ from the reference's `>`, in any float type; and every speed bucket has rows."""
    for name in FIXTURES:
        speed, e = _stored_rows(name)
        rel = lambda v, edge: float(np.abs(v - edge).min() / edge)      # noqa: E731
        margins = [rel(speed, x) for x in cr.SPEED_EDGES] + [rel(e, x) for x in cr.ERROR_EDGES]
        buckets = [int(((speed >= lo) & (speed < hi)).sum()) for lo, hi in zip((0.0,) + cr.SPEED_EDGES, cr.SPEED_EDGES + (np.inf,))]
        print(f"{name}: relative margins speed {margins[:2]}, e {margins[2:]}, rows per speed bucket {buckets}")
        assert min(margins[:2]) > 1e-6 and min(margins[2:]) > 1e-9
        assert all(b > 0 for b in buckets)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_marginals_equal_the_reference(name):
    """72 comparisons in all: four files x three settings x six classes.  Row counts exactly <setting>_num, sum / count within
    1e-12 (relative) of <setting>_avg[:, 0] -- numpy's pairwise mean against sequential sums of at most 63 276 values."""
    s, pred = cr.fixture_sample(name)
    worst = 0.0
    for setting in ar.SETTINGS:
        c = cr.table(ar.setting_args(setting), s, pred, s["classes"])
        assert c.outside == 0
        worst = max(worst, cr.check_against_recorded(name, setting, c.counts, c.sequential("e")))
    print(f"{name}: largest relative difference of a mean {worst:.3e}")


# ---- ClassTable -----------------------------------------------------------------------------------------------------------
def _product_table(c):
    from icp_flow_amd import utils_eval
    return utils_eval.ClassTable(c.counts, c.sequential("e"), c.sequential("speed"), c.kept0)


def test_meta_threeway_and_the_printed_lines():
    from icp_flow_amd import utils_eval
    s, pred = cr.fixture_sample("g15_argo_f32_int")
    c = cr.table(ar.setting_args("argo"), s, pred, s["classes"])
    t = _product_table(c)
    # words <-> table, add
    again = utils_eval.ClassTable.from_words(t.words(), 33, 3, 3, kept0=t.kept0)
    assert np.array_equal(again.counts, t.counts) and again.esum.tobytes() == t.esum.tobytes() and again.ssum.tobytes() == t.ssum.tobytes()
    twice = utils_eval.ClassTable.zeros(33, 3, 3).add(t).add(t)
    assert np.array_equal(twice.counts, 2 * t.counts) and np.array_equal(twice.esum, t.esum + t.esum) and twice.kept0 == 2 * t.kept0
    with pytest.raises(ValueError):
        t.add(utils_eval.ClassTable.zeros(2, 1, 1))
    # meta: rows in ascending order, the rest OTHER
    meta = t.meta(utils_eval.ARGO_META_GROUPS)
    assert meta.names == ("BACKGROUND", "PEDESTRIAN", "SMALL_MOVERS", "LARGE_MOVERS", "OTHER") and meta.counts.shape == (5, 3, 3)
    assert int(meta.counts.sum()) == int(t.counts.sum())
    for k, rows in enumerate(list(utils_eval.ARGO_META_GROUPS.values()) + [(1, 2, 11, 32)]):
        assert np.array_equal(meta.counts[k], t.counts[list(rows)].sum(axis=0))
        acc = np.zeros(3)
        for r in sorted(rows):
            acc = acc + t.esum[r]
        assert meta.esum[k].tobytes() == acc.tobytes()
    with pytest.raises(ValueError):
        t.meta({"A": (1, 2), "B": (2,)})
    # three-way: FD / FS / BS are the means behind dynamic_fg / static_fg / static_bg
    tw = t.threeway()
    m = cr.marginals(t.counts, t.esum)
    for part, cls in (("FD", "dynamic_fg"), ("FS", "static_fg"), ("BS", "static_bg")):
        n, total = m[cls]
        assert tw["n_" + part] == n and tw[part] == total / n
    assert tw["mean"] == (tw["FD"] + tw["FS"] + tw["BS"]) / 3.0
    assert tw["n_BD"] == m["dynamic"][0] - m["dynamic_fg"][0] and tw["n_BD"] > 0
    # an empty component is NaN, and so is the mean
    still = utils_eval.ClassTable(t.counts * np.array([1, 0, 0])[None, :, None], t.esum * np.array([1, 0, 0]), t.ssum * np.array([1, 0, 0]))
    tw0 = still.threeway()
    assert math.isnan(tw0["FD"]) and math.isnan(tw0["mean"]) and tw0["n_FD"] == 0 and tw0["FS"] == tw["FS"] and tw0["BS"] == tw["BS"]
    # the lines: one per non-empty (meta category, speed bucket), the fine rows after them, the three-way line last
    text = utils_eval.format_class_table(t).split("\n")
    assert len(text) == 1 + int((meta.counts.sum(axis=2) > 0).sum()) + 1
    n, es, ss, cnt = int(meta.counts[0, 1].sum()), meta.esum[0, 1], meta.ssum[0, 1], meta.counts[0, 1]
    want = f"n: {n:8d}, EPE3D: {es / n:.6f}, speed: {ss / n * 10.0:.4f} m/s, e<0.05/e<0.1/rest: " + " ".join(f"{x / n:.4f}" for x in cnt)
    line = [x for x in text if "BACKGROUND" in x and "[0.5, 2) m/s" in x]
    assert len(line) == 1 and line[0].endswith(want)
    assert text[-1].startswith(f"three-way EPE: {tw['mean']:.6f}, FD: {tw['FD']:.6f} (n {tw['n_FD']})") and text[-1].endswith(f"in no component: {tw['n_BD']}")
    fine = utils_eval.format_class_table(t, fine=True).split("\n")
    assert len(fine) == len(text) + 1 + int((t.counts.sum(axis=2) > 0).sum()) and any("REGULAR_VEHICLE" in x for x in fine) and fine[-1] == text[-1]
    assert not any("REGULAR_VEHICLE" in x for x in text)


# ---- saving -------------------------------------------------------------------------------------------------------------
def test_save_path_rule():
    from icp_flow_amd import frame_pairs
    f = frame_pairs.flow_file
    assert f("/d/val/x.npz") == "/d/val_icp_flow_ego/x.npz" and f("/d/val/x.npz", estimated_poses=True) == "/d/val_icp_flow/x.npz"
    assert f("/d/val_zero_flow/log/x.npz") == "/d/val_icp_flow_ego_zero_flow/log/x.npz"
    assert f("/d/train_zero_flow/log/x.npz", True) == "/d/train_icp_flow_zero_flow/log/x.npz"
    assert f("/latest/test/x.npz") == "/latest/test_icp_flow_ego/x.npz"           # a component, never a substring
    assert f("/val/a/val_zero_flow/x.npz") == "/val/a/val_icp_flow_ego_zero_flow/x.npz"   # the last one wins
    for path in ("/d/validation/x.npz", "/d/latest/x.npz", "x.npz", "/d/val.npz"):
        with pytest.raises(ValueError, match=os.path.basename(path).replace(".", r"\.")):
            f(path)


def test_metrics_file_keys_and_shapes(tmp_path):
    from icp_flow_amd import utils_eval
    meters = utils_eval.new_metric_table(2)
    for k, name in enumerate(meters):
        for j in range(k % 3):
            meters[name].update(0.1 * j, np.float32(0.5), np.float32(0.6), np.float32(0.2), np.float32(0.1), 10 + j)
    path = str(tmp_path / "metrics_argo_val_x.npz")
    keys = utils_eval.save_metrics_file(path, meters, 2)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(keys) and len(keys) == 18 * 5
        for k, name in enumerate(meters):
            for prefix, field in (("EPE3D", "epe"), ("ACC3DS_", "accs"), ("ACC3DR_", "accr"), ("OUTLIER_", "outlier"), ("ROUTLIER_", "Routlier")):
                a = z[prefix + name]
                assert a.shape == (1, k % 3) and a.dtype == np.float64
                assert np.array_equal(a[0], np.asarray(getattr(meters[name], field + "_data"), np.float64))
    assert "EPE3Doverall_0" in keys and "ACC3DS_dynamic_fg_2" in keys and "ROUTLIER_static_bg_1" in keys


# ---- ranks ----------------------------------------------------------------------------------------------------------------
CLASS_SHAPE = (33, 3, 3)


def _five_records():
    """Five files' records: tables of the seqeval restatement on a g13 sample (F = 3) under five predictions, class tables of the
    class restatement on a g15 sample under five predictions -- two of them empty (a file whose every row was cropped away
    from the classes' point of view)."""
    from icp_flow_amd import frame_pairs, utils_eval
    g = sr.load("g13_seqeval_f3_f64")
    args = sr.crop_args(g, 0)
    data = sr.sample(g)
    s, pred_c = cr.fixture_sample("g15_argo_f64")
    rng = np.random.default_rng(16)
    records = []
    for k in range(5):
        pred = (g["pred_flow"] + rng.normal(scale=0.05 * k, size=g["pred_flow"].shape)).astype(np.float32)
        table, esum, kept0 = sr.table_numpy(args, data, pred)
        table[:, :, 1] = esum.view(np.int64)
        if k in (1, 4):
            classes = utils_eval.ClassTable.zeros(*CLASS_SHAPE)
        else:
            c = cr.table(ar.setting_args("argo"), s, (pred_c + rng.normal(scale=0.02 * k, size=pred_c.shape)).astype(np.float32), s["classes"])
            classes = utils_eval.ClassTable(c.counts, c.sequential("e"), c.sequential("speed"), c.kept0)
        records.append(frame_pairs.sequence_record(k, 3, table, kept0, 2, (1000.0 + k, 100.0 + k, 0.0), classes))
    return args, np.stack(records)


def _meter_bytes(metrics, classes):
    from icp_flow_amd import utils_eval
    out = {"class_words": classes.words(), "class_kept0": np.array(classes.kept0)}
    for name, m in metrics.items():
        out[name + "/num"] = np.asarray(m.num, np.float64)
        out[name + "/num_data"] = np.asarray(m.num_data, np.float64)
        for metric in utils_eval.METRIC_NAMES:
            for field in ("_sum", "_avg", "_data"):
                out[f"{name}/{metric}{field}"] = np.asarray(getattr(m, metric + field), np.float64)
    return out


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merge_worker(rank, world, port, records_path, out_dir):
    import torch.distributed as dist
    from icp_flow_amd import frame_pairs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    with np.load(records_path) as z:
        records, args = z["records"], SimpleNamespace(num_frames=int(z["num_frames"]))
    mine = [records[k] for k in range(len(records))][rank::world]
    metrics, classes, heads = frame_pairs.merge_sequence_records(args, mine, len(records), rank, world, class_shape=CLASS_SHAPE)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), heads=heads, **_meter_bytes(metrics, classes))
    dist.destroy_process_group()


def test_sharded_replay_is_bit_identical_to_a_single_process(tmp_path):
    """merge_sequence_records under gloo on 1, 2 and 3 ranks (shares 5; 3 + 2; 2 + 2 + 1): every rank's meters (num, every
    *_sum, *_avg, *_data) and class table equal the plain replay in file order bit for bit."""
    import torch.multiprocessing as mp
    from icp_flow_amd import frame_pairs, utils_eval
    args, records = _five_records()
    # the single process: update_meters and ClassTable.add, file after file
    want_m, want_c = utils_eval.new_metric_table(3), utils_eval.ClassTable.zeros(*CLASS_SHAPE)
    H = frame_pairs.RECORD_HEAD
    for r in records:
        table = r[H:H + 108].reshape(3, 6, 6).copy()
        utils_eval.update_meters(args, want_m, table, np.ascontiguousarray(table[:, :, 1]).view(np.float64), int(r[1]))
        want_c.add(utils_eval.ClassTable.from_words(r[H + 108:], *CLASS_SHAPE, kept0=int(r[1])))
    want = _meter_bytes(want_m, want_c)
    assert want_m["overall_0"].num > 0 and len(want_m["overall_3"].epe_data) == 5 and int(want_c.counts.sum()) > 0
    records_path = str(tmp_path / "records.npz")
    np.savez(records_path, records=records, num_frames=np.array(3))
    for world in (1, 2, 3):
        out_dir = str(tmp_path / f"world{world}")
        os.makedirs(out_dir)
        mp.spawn(_merge_worker, args=(world, _free_port(), records_path, out_dir), nprocs=world, join=True)
        for rank in range(world):
            with np.load(os.path.join(out_dir, f"rank{rank}.npz")) as z:
                assert sorted(z.files) == sorted(list(want) + ["heads"])
                for k, v in want.items():
                    assert z[k].shape == v.shape and z[k].tobytes() == v.tobytes(), (world, rank, k)
                assert np.array_equal(z["heads"], records[:, :H])
    # a record too many, a record of the wrong length, a file missing
    with pytest.raises(ValueError):
        frame_pairs.merge_sequence_records(args, list(records), 4, class_shape=CLASS_SHAPE)
    with pytest.raises(ValueError):
        frame_pairs.merge_sequence_records(args, [records[0][:-1]], 1, class_shape=CLASS_SHAPE)
    with pytest.raises(RuntimeError, match="do not cover"):
        frame_pairs.merge_sequence_records(args, list(records[1:]), 5, class_shape=CLASS_SHAPE)

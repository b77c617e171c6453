"""bench.py --gpus N starts its own ranks when no launcher did: the launcher, the
rendezvous on 127.0.0.1, the contiguous shards and the one all_gather of [B,26] rows, driven over gloo on CPU tensors
(`--launch-selftest`: no GPU work, made-up rows), and the refusal on a box with too few devices."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_self_launch_two_gloo_ranks_print_one_json_line():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "0", "--pairs", "101", "--launch-selftest"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                      # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2
    assert out["config"]["pairs_per_gpu"] == [51, 50] and out["config"]["pairs_total"] == 101
    assert out["gather_check"] == {"rows": [101, 26], "identical_to_all_ranks_rows": True, "backend": "gloo", "rccl_library": None}
    # every N > 1 line names its own single-GPU point (the same workload on one GPU) and the efficiency against it
    assert "n1_same_workload" in out and out["n1_same_workload"]["pairs"] == 101 and "scaling_efficiency" in out


def test_self_launch_refuses_when_devices_are_missing():
    """More ranks than devices: a plain message about devices, not a launcher error (and nothing is spawned)."""
    n = torch.cuda.device_count() + 1 if torch.cuda.device_count() >= 1 else 2
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--steps", "2"], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert f"needs {n} devices, found {torch.cuda.device_count()}" in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


def test_stream_workload_eight_gloo_ranks_uneven_shares():
    """`bench.py --gpus 8 --workload stream` -- 13 frame pairs dealt round-robin to eight self-launched
    ranks (shares 2,2,2,2,2,1,1,1), the one all_reduce per step, run_stream's summary and the N = 1 point (`--full`); gloo, a
    stand-in for the registration (`--launch-selftest`).  One JSON line naming the stream, n_gpus and the per-rank counts."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--workload", "stream", "--frame-pairs", "13", "--steps", "2", "--warmup", "1",
                        "--launch-selftest", "--full"], env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["steps"] == 2 and out["unit"] == "ms/frame-pair" and out["higher_is_better"] is False
    assert "frame-pair stream" in out["config"]["workload"]
    assert out["config"]["frame_pairs_per_gpu"] == [2, 2, 2, 2, 2, 1, 1, 1] and out["config"]["frame_pairs_total"] == 13
    assert out["reduce_check"] == {"frame_pairs_counted_by_all_ranks": 13, "equals_sum_of_shares": True, "backend": "gloo", "rccl_library": None}
    assert out["accuracy"]["frame_pairs"] == 13 and out["accuracy"]["epe"] == 0.0
    assert out["n1_same_workload"]["frame_pairs"] == 13 and out["n1_same_workload"]["unit"] == "ms/frame-pair" and out["scaling_efficiency"] is not None


def test_stream_workload_refuses_when_devices_are_missing():
    n = torch.cuda.device_count() + 1 if torch.cuda.device_count() >= 1 else 2
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--workload", "stream", "--steps", "1"], env=_env(), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0
    assert f"needs {n} devices, found {torch.cuda.device_count()}" in r.stderr, r.stderr[-2000:]


def test_stream_dump_outputs_are_the_last_steps_results(tmp_path):
    """`--dump-outputs DIR`: rank 0 writes what its frame pairs returned in the last timed step, in stream order, as float32 /
    float64 .npy files; a plain run (no `--full`) carries no accuracy pass and no N = 1 point."""
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--workload", "stream", "--frame-pairs", "5", "--steps", "3", "--warmup", "0",
                        "--launch-selftest", "--dump-outputs", str(out_dir)], env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] >= 0 and out["reduce_check"]["equals_sum_of_shares"]
    assert "accuracy" not in out and "n1_same_workload" not in out
    from icp_flow_amd import synthetic
    mine = [synthetic.make_frame_pair(seed=k, n_objects=3, n_max=60, n_background=50) for k in (0, 2, 4)]   # rank 0's round-robin share
    flow = np.load(out_dir / "flow.npy")
    assert flow.dtype == np.float32 and np.array_equal(flow, np.concatenate([d["gt_flow"] for d in mine]).astype(np.float32))
    counts = np.load(out_dir / "pairs_per_frame_pair.npy")
    assert counts.dtype == np.float64 and counts.tolist() == [len(d["points_src"]) % 7 + 1 for d in mine]
    assert np.load(out_dir / "pairs.npy").shape == (int(counts.sum()), 10)
    assert np.load(out_dir / "transformations.npy").shape == (int(counts.sum()), 4, 4)


def test_dump_outputs_samples_rows_past_the_limit(tmp_path, monkeypatch):
    """Past the size limit the largest array is cut to a seeded sample of its rows (indices beside it), the same in every run."""
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.arange(3000, dtype=np.float64).reshape(1000, 3) * 0.5
    small = torch.arange(4, dtype=torch.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "big_rows.npy", "small.npy"]
    assert sum(x.nbytes for x in got.values()) <= 4096
    rows = got["big_rows.npy"].astype(np.int64)
    assert len(rows) > 1 and np.all(np.diff(rows) > 0) and np.array_equal(got["big.npy"], big[rows])
    assert got["small.npy"].dtype == np.float64 and got["small.npy"].tolist() == [0, 1, 2, 3]
    for f, x in got.items():
        assert np.array_equal(np.load(tmp_path / "b" / f), x)

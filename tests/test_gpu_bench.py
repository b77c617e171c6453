"""The headline line of bench.py on the box it will run on: a plain `--gpus 1` run times exactly `--steps` steps, prints the
headline fields and nothing that needs runs of its own (those are `--full`), and `--dump-outputs` writes what the last timed
step returned -- hist_icp's transforms and iteration count for config 2's seeded batch, as this process computes them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def test_plain_line_and_dumped_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["metric"] == "cluster-pair ICP registrations/sec" and out["unit"] == "registrations/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(256 / out["ms_per_step"] * 1e3, rel=1e-3)
    assert out["roofline"]["steps_of_the_timed_region"] == 3
    assert not {"cpu_baseline", "extras", "config4_on_one_gpu"} & set(out)

    from types import SimpleNamespace
    from icp_flow_amd import synthetic, utils_match
    S, D, _ = synthetic.make_batch(256, 1024, seed=0, first=0)
    dev = torch.device("cuda", 0)
    args = SimpleNamespace(thres_dist=0.1, translation_frame=2.0, chunk_size=50, max_points=1024, icp_max_iterations=50,
                           icp_stop_mode="reference")
    T, iters = utils_match.hist_icp(args, torch.from_numpy(S).to(dev), torch.from_numpy(D).to(dev), return_iterations=True)
    got_T, got_it = np.load(out_dir / "transformations.npy"), np.load(out_dir / "icp_iterations.npy")
    assert got_T.dtype == np.float32 and got_T.shape == (256, 4, 4)
    np.testing.assert_allclose(got_T, T.cpu().numpy(), atol=1e-5, rtol=0)
    assert got_it.dtype == np.float64 and got_it.tolist() == [int(iters.item())]

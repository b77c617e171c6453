"""icpflow_match_eval (row a-12) on its own against tests/match_eval_restatement.py: every case of tests/match_eval_cases.py -- the
scans with one, two and four queries per lane, both instantiations of the sweeps with their windows, shared windows and shared
full scans, the poses, the threshold, duplicated targets, empty and one-point clouds -- and every sweep case again as scans.

Per pair: inliers, ratios and ious array_equal; errors and translations inside the interval that the order of the library's float64
sums allows (derived: match_eval_restatement.sum_bounds), with the number of error values that are not bit-equal printed; rotations
within ROT_BOUND of the float64 evaluation of the same float32 entries.  The guards of the exactly sized 0xFF workspace and of every
output are intact, a rerun and a run on a second stream are bit-identical (tests/match_eval_device.py).

ROT_BOUND: the largest difference measured on an MI355X over this file's poses was 9.16e-6 degrees (ROT_MEASURED; COVERAGE.md, row
a-12); asserted at four times that, below the 1e-4 degrees of the rest of the suite."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_eval_cases as mc            # noqa: E402
import match_eval_device as md           # noqa: E402
import match_eval_restatement as mr      # noqa: E402

F = np.float32
ROT_MEASURED = 9.16e-6
ROT_BOUND = 4 * ROT_MEASURED
assert ROT_BOUND <= 1e-4


@pytest.mark.parametrize("name,no_eval_sweep", mc.runs(), ids=[n + ("-as_scans" if s else "") for n, s in mc.runs()])
def test_match_eval_against_the_restatement(name, no_eval_sweep):
    c = mc.get(name)
    recs, want = mc.restated(name)
    got = md.run(c, no_eval_sweep)
    unequal, worst = md.compare(got, recs, want, c["T"], ROT_BOUND, name)
    print(f"{name}{' as scans' if no_eval_sweep else ''}: {mc.paths(c, no_eval_sweep)['kernel']}, {unequal} of {2 * len(recs)} error values not bit-equal, "
          f"rotations within {worst:.3g} degrees")
    assert md.same_bits(md.run(c, no_eval_sweep), got), "a rerun differs"
    assert md.same_bits(md.run(c, no_eval_sweep, stream=torch.cuda.Stream()), got), "a run on a second stream differs"


@pytest.mark.parametrize("name", ["empty_and_one_point_N300", "empty_and_one_point_N2049"])
def test_empty_sides_by_the_contract(name):
    """A non-empty side against an empty one has the error +inf and no inliers, by the scans and by the sweeps alike; an empty query
    side has NaN, as the oracle gives.  (The reference's un-lengthed search reports the distance to the pads, 173205104: COVERAGE.md,
    named deviations.)"""
    got = md.run(mc.get(name))
    e = got["errors"]
    assert e[0, 0] == np.inf and np.isnan(e[0, 1]), e[0]            # (200, 0)
    assert np.isnan(e[1, 0]) and e[1, 1] == np.inf, e[1]            # (0, 200)
    assert np.isnan(e[2]).all(), e[2]                               # (0, 0)
    assert (got["inliers"][:3] == 0).all() and got["ratios"][0, 0] == 0 and got["ious"][0, 0] == 0


def test_rotations_exact_cases():
    c = mc.get("rotations_exact_N16")
    r = dict(zip(c["names"], md.run(c)["rotations"]))
    assert np.array_equal(md.bits(r["identity"]), md.bits(np.array([0.0, -0.0, 0.0], F))), r["identity"]      # (0, -0, 0), as the oracle prints
    for n in ("m8_above_1", "m8_below_minus_1"):                    # NaN in the middle angle and nowhere else
        assert np.isnan(r[n][1]) and not np.isnan(r[n][[0, 2]]).any(), (n, r[n])
    for n, M in zip(c["names"], c["T"]):
        if n.startswith("half_turn"):                               # atan2(+-0, -1) = +-pi
            assert np.array_equal(md.bits(r[n]), md.bits(mr.rotations32(M))), (n, r[n], mr.rotations32(M))
    assert r["half_turn_plus_zero"][0] == F(180.0) and r["half_turn_minus_zero"][0] == F(-180.0)


@pytest.mark.parametrize("N", [300, 2049])
def test_hist_icp_eval_metrics_against_the_restatement(N):
    """icpflow_hist_icp_eval: the metrics it reports are the restatement's at the transforms it returns -- sweeps at any width, on the
    clouds hist_icp sorted by role (swap flags, direction keys), dispatched through the pair table in the order of the plan."""
    from icp_flow_amd import utils_match
    from oracle import reference_path as rp
    S, D = mc.hist_icp_eval_batch(N)
    args = rp.default_args(max_points=N)
    T, ev = utils_match.hist_icp_eval(args, torch.from_numpy(S).to(md.DEV), torch.from_numpy(D).to(md.DEV))
    T = T.cpu().numpy()
    assert np.isfinite(T).all()
    got = {k: v.cpu().numpy() for (k, _), v in zip(md.OUTPUTS, ev)}
    recs, want = mr.batch(S, D, T, args.thres_dist)
    unequal, worst = md.compare(got, recs, want, T, ROT_BOUND, f"hist_icp_eval N={N}")
    print(f"hist_icp_eval N={N}: {unequal} of {2 * len(recs)} error values not bit-equal, rotations within {worst:.3g} degrees")
    assert (got["inliers"][:, 0] > 0).all()              # (the registration found every pair: the metrics are of overlapping clouds)

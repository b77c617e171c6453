"""The registrations that keep score_pick_kernel (api.hip pick_in_icp, icp.hip icp_pick_in_icp: teams of workgroups, one launch
per iteration beyond 128 iterations, a stage's first half that returns without its ICP launch) against the ones whose ICP launch
picks the initial poses itself: the same results, selected by the library's existing options."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, frame_pairs, synthetic, utils_hist, utils_icp, utils_match  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def same(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def composition(a, s, d):
    init = utils_hist.estimate_init_pose(a, s, d)
    return utils_icp.apply_icp(a, s, d, init, return_iterations=True)


def test_teams_keep_the_kernel_and_no_teams_folds():
    """Four pairs of 1100 points leave most of the GPU idle: the ICP launch takes teams of workgroups and the kernel stays;
    ICPFLOW_OPT_NO_TEAMS gives every pair one workgroup, whose wave 0 picks.  Each equals the unfolded composition under the same
    option bit for bit; between them the order of a team's sums differs, nothing else: the same iteration count, poses to
    rounding."""
    S, D, _ = synthetic.make_batch(4, 1100, seed=21)
    a = rp.default_args(max_points=1100, icp_max_iterations=50)
    s, d = G(S), G(D)
    res = []
    for no_teams in (False, True):
        with _lib.options(no_teams=no_teams):
            T, it = composition(a, s, d)
            Tf, itf = utils_match.hist_icp(a, s, d, return_iterations=True)
        assert int(itf) == int(it) and same(Tf, T), no_teams
        res.append((Tf.cpu().numpy(), int(itf)))
    assert res[0][1] == res[1][1]
    np.testing.assert_allclose(res[0][0], res[1][0], atol=2e-6)


def test_more_than_128_iterations_one_launch_per_iteration():
    """A cap of 150 iterations takes one launch per iteration, in front of which the kernel picks; the batch stops long before
    128, where the single speculative launch (cap 128: its wave 0 picks) stops too -- the same transforms and count, and both
    those of the unfolded composition."""
    S, D, _ = synthetic.make_batch(6, 700, seed=33)
    s, d = G(S), G(D)
    a150 = rp.default_args(max_points=700, icp_max_iterations=150)
    a128 = rp.default_args(max_points=700, icp_max_iterations=128)
    T150, it150 = utils_match.hist_icp(a150, s, d, return_iterations=True)
    T128, it128 = utils_match.hist_icp(a128, s, d, return_iterations=True)
    assert 1 < int(it128) < 128
    assert int(it150) == int(it128) and same(T150, T128)
    Tc, itc = composition(a150, s, d)
    assert int(itc) == int(it150) and same(Tc, T150)


def test_staged_begin_and_finish_against_one_call_per_stage():
    """A frame pair through icpflow_track_frame: with the stages overlapped, stage 2 registers through
    icpflow_register_stage_begin / _finish (its first half enqueues the ICP launch where it can be split off, and returns
    without one where it cannot: the kernel stays); without the overlap every stage is one call.  Clusters of 600 to 1000
    points (sweep scoring: the launches pick).  Pairs, transforms and flow bit for bit."""
    d = synthetic.make_frame_pair(seed=12, n_objects=8, n_min=600, n_max=1000, n_background=600)
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    out = []
    for overlap in (True, False):
        a = frame_pairs.default_args(max_points=1024)
        a.stage_overlap = overlap
        r = frame_pairs.register_frame_pair_native(a, fp, DEV)
        assert frame_pairs._served(r)
        torch.cuda.synchronize()
        out.append(r)
    assert len(out[0]["pairs"]) >= 4
    for k in ("pairs", "transformations", "flow"):
        assert same(out[0][k], out[1][k]), k

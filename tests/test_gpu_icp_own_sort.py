"""The ICP entry points that sort for themselves (icpflow_icp, icpflow_apply_icp: launch_icp finds the clouds unsorted and
calls the one sort launcher of icp_prep.hip, which hist_icp's side stream and match_eval call too) on both sides of
kChunkSortMinN = 4096 points -- one workgroup per cloud below, the chunked sort of sort.hip above -- without a pre-pose
(icpflow_icp) and with one (icpflow_apply_icp's initial poses).  Two full pairs per case; transforms, rmse and iteration
counts bit for bit as recorded from the library before the sort launches of launch_icp and launch_sort_clouds_soa became
one function (tests/golden/g17_icp_own_sort.npz; inputs are synthetic.make_batch's, rebuilt here)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import synthetic, utils_icp  # noqa: E402
from icp_flow_amd import utils_icp_pytorch3d as p3d  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")
SIZES = (4090, 4100)
ITERS = 12


def run(N):
    """-> {name: array} of both entry points on the two pairs of padded length N."""
    S, D, _ = synthetic.make_batch(2, N, seed=170 + N)
    s, d = torch.from_numpy(S).to(DEV), torch.from_numpy(D).to(DEV)
    sol = p3d.iterative_closest_point(s, d, max_iterations=ITERS)
    init = torch.eye(4, device=DEV).repeat(2, 1, 1)
    init[0, :3, 3] = torch.tensor([0.05, -0.03, 0.01], device=DEV)
    init[1, :3, 3] = torch.tensor([-0.04, 0.06, 0.0], device=DEV)
    a = rp.default_args(max_points=N, icp_max_iterations=ITERS)
    T, it = utils_icp.apply_icp(a, s, d, init, return_iterations=True)
    return {"icp_R": sol.RTs.R.cpu().numpy(), "icp_T": sol.RTs.T.cpu().numpy(), "icp_rmse": sol.rmse.cpu().numpy(),
            "apply_T": T.cpu().numpy(), "apply_iters": it.cpu().numpy()}


@pytest.mark.parametrize("N", SIZES)
def test_own_sort_on_both_sides_of_the_chunked_sort(N, golden):
    want = golden("g17_icp_own_sort")
    got = run(N)
    for k, v in got.items():
        w = want[f"n{N}_{k}"]
        assert np.isfinite(v).all(), k
        assert v.dtype == w.dtype and np.array_equal(v, w), (N, k, np.abs(v.astype(np.float64) - w).max())

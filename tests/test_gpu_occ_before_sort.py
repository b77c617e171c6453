"""The occupancy grids of hist_icp's scoring are built from the clouds as they come in, in front of the side stream's axis sort
(nn.hip occ_build_kernel<true>), where one workgroup sorts a cloud (N <= 4096); from the sorted images behind the sort otherwise and
without the side stream.  A grid is a function of the points as a set, so nothing may change: on ragged batches -- rows with a
flag of zero behind the valid ones, pairs whose roles are swapped, clouds far from the origin, an empty cloud -- transforms and
iteration counts are bit for bit those of the grids from the sorted images (ICPFLOW_OPT_NO_SIDE_STREAM), of the sweeps without the
grids (ICPFLOW_OPT_NO_SCORE_PREBOUND) and of every scan run to its end (ICPFLOW_OPT_NO_SCORE_PRUNE): a grid that missed a point
would bound a scan too high and prune a candidate that the full scans keep."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, synthetic, utils_match  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")
VARIANTS = ({"no_side_stream": True}, {"no_score_prebound": True}, {"no_score_prune": True})


def _bits(t):
    return t.contiguous().view(torch.int32)


# widths: below and at the single-workgroup sort's limit (grids first), above it (grids behind the chunked sort)
@pytest.mark.parametrize("N,B,far", [(520, 24, False), (1024, 24, True), (4096, 6, False), (5000, 6, True)])
def test_grids_from_the_raw_clouds_change_nothing(N, B, far):
    rng = np.random.default_rng(N)
    S, D, _ = synthetic.make_batch(B, N, seed=N + 1, ragged=True, n_min=40)
    S[1], D[1] = D[1].copy(), S[1].copy()                     # a pair the other way round (roles follow the lengths)
    S[2, :, 3] = 0.0                                          # ... and one with an empty cloud
    if far:
        off = rng.uniform(-900, 900, (B, 1, 3)).astype(np.float32)
        S[:, :, :3] += off * (S[:, :, 3:4] > 0)
        D[:, :, :3] += off * (D[:, :, 3:4] > 0)
    a = rp.default_args(max_points=N)
    s, d = torch.from_numpy(S).to(DEV), torch.from_numpy(D).to(DEV)
    T1, it1 = utils_match.hist_icp(a, s, d, return_iterations=True)
    for v in VARIANTS:
        with _lib.options(**v):
            T0, it0 = utils_match.hist_icp(a, s, d, return_iterations=True)
        assert int(it0) == int(it1), v
        assert torch.equal(_bits(T0), _bits(T1)), v

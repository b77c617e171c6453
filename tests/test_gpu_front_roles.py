"""hist_icp's axis sort and occupancy grids run as workgroups of the vote's own launch, in front of the vote's (hist.hip
front_roles_kernel), where the vote gives four waves to every 64 rows and one workgroup sorts a cloud (1024 <= N <= 4096): 512
threads sort a cloud instead of 1024, the two grids of a pair are built by the two halves of one eight-wave workgroup, every role carves
the vote's dynamic LDS, and the lengths and roles come from the z sort instead of being counted again.  Sorting is a function of
the keys and a grid one of the points as a set, so nothing may change: on ragged batches -- rows with a flag of zero behind the
valid ones, a pair whose roles are swapped, an empty cloud, clouds of a single row -- transforms and iteration counts are bit for
bit those of the side stream's two launches (ICPFLOW_OPT_NO_FRONT_ROLES), of everything on one stream
(ICPFLOW_OPT_NO_SIDE_STREAM) and of the sweeps without the grids (ICPFLOW_OPT_NO_SCORE_PREBOUND: the launch then holds no grid
workgroups)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, synthetic, utils_match  # noqa: E402
from oracle import reference_path as rp  # noqa: E402

DEV = torch.device("cuda:0")
VARIANTS = ({"no_front_roles": True}, {"no_side_stream": True}, {"no_score_prebound": True})


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ragged(B, N, far=False, empty=True):
    S, D, _ = synthetic.make_batch(B, N, seed=N + B, ragged=True, n_min=1)
    k = 1 % B
    S[k], D[k] = D[k].copy(), S[k].copy()                     # a pair the other way round (roles follow the lengths)
    if empty:
        S[2 % B, :, 3] = 0.0                                  # ... and one with an empty cloud
    if far:
        off = np.random.default_rng(N).uniform(-900, 900, (B, 1, 3)).astype(np.float32)
        S[:, :, :3] += off * (S[:, :, 3:4] > 0)
        D[:, :, :3] += off * (D[:, :, 3:4] > 0)
    return S, D


def _sized(N, sizes):
    """Pairs of exactly these (src, dst) row counts."""
    S = np.empty((len(sizes), N, 4), np.float32)
    D = np.empty((len(sizes), N, 4), np.float32)
    for i, (ns, nd) in enumerate(sizes):
        S[i], D[i], _ = synthetic.make_pair(i, max(ns, 1), max(nd, 1), N, seed=N)
        if ns == 0:
            S[i, :, 3] = 0.0
        if nd == 0:
            D[i, :, 3] = 0.0
    return S, D


def _check(run, variants=VARIANTS):
    ref = run()
    for v in variants:
        with _lib.options(**v):
            got = run()
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert torch.equal(_bits(g), _bits(r)), v


def _hist_icp(a, s, d):
    return lambda: utils_match.hist_icp(a, s, d, return_iterations=True)


# (1024, 3): the smallest width of the <512, 4> vote, one exchange per thread.  (1024, 1): the last pair's overflow bins with the
# block offset in play -- a batch of one pair cannot both vote and hold an empty cloud, so it runs twice: with the empty cloud, and
# without it (the pair that votes).  (4096, 4): 32 KiB of keys in the vote's buffer.  (4100, 4): beyond what one workgroup sorts --
# the side stream's chunked sort, as before.  (1024, 24) far: clouds 900 m from the origin, grids that refuse per cloud.
@pytest.mark.parametrize("N,B,far,empty", [(1024, 3, False, True), (1024, 1, False, True), (1024, 1, False, False), (4096, 4, False, True),
                                           (4100, 4, False, True), (1024, 24, True, True)])
def test_front_roles_change_nothing(N, B, far, empty):
    S, D = _ragged(B, N, far, empty)
    a = rp.default_args(max_points=N)
    _check(_hist_icp(a, torch.from_numpy(S).to(DEV), torch.from_numpy(D).to(DEV)))


def test_networks_of_64_to_2048():
    """Clouds of 1, 64, 65, 1024 and 1100 rows in a batch 1100 wide: sort networks of 64, 128, 1024 and 2048 keys on 512 threads
    (one exchange per thread up to 1024 keys, two at 2048), every length in both roles; pair 1 is swapped by its lengths, pair 2
    has an empty src cloud."""
    N = 1100
    S, D = _sized(N, [(1, 1100), (1024, 64), (0, 65), (65, 1024), (1100, 1100)])
    a = rp.default_args(max_points=N)
    _check(_hist_icp(a, torch.from_numpy(S).to(DEV), torch.from_numpy(D).to(DEV)))


def test_front_roles_through_hist_icp_many():
    N = 1024
    a = rp.default_args(max_points=N)
    batches = [_ragged(B, N) for B in (3, 5)]
    ss = [torch.from_numpy(S).to(DEV) for S, _ in batches]
    dd = [torch.from_numpy(D).to(DEV) for _, D in batches]

    def run():
        Ts, its = utils_match.hist_icp_many(a, ss, dd, return_iterations=True)
        return list(Ts) + list(its)
    _check(run)


def test_front_roles_through_hist_icp_eval():
    """Transforms and iteration count against every variant; the metrics against the side stream's launches, whose sorted clouds
    they reuse (the metrics of a pair with an empty cloud are not specified, and differ between one stream and two as before)."""
    N = 1024
    a = rp.default_args(max_points=N)
    S, D = _ragged(6, N)
    s, d = torch.from_numpy(S).to(DEV), torch.from_numpy(D).to(DEV)

    def run(metrics=False):
        T, ev, it = utils_match.hist_icp_eval(a, s, d, return_iterations=True)
        return [T, it, *ev] if metrics else [T, it]
    _check(run)
    _check(lambda: run(True), ({"no_front_roles": True},))

"""GPU: the workspace contract of icpflow_cluster_pcd and icpflow_track_frame_points, after tests/test_gpu_workspace_contract.py:
the call runs the way a C caller runs it -- on EXACTLY icpflow_cluster_pcd_workspace_bytes() bytes filled with a poison, between
guard bytes, outputs between guards as well -- and gives the bits of the ordinary run; the same with the base 16 bytes further;
`need - 1` is refused with ICPFLOW_E_WORKSPACE before anything is written.  Both branches.

Who writes what before it is read (csrc/clusterpcd.hip): pts, mask and the two counters: stack_kernel; labels, counts and the
number of clusters: icpflow_dbscan's kernels (counts cleared by its first); keep[0..C): keep_rank_kernel before finish_kernel
reads keep[label]; HDBSCAN: core2, the edges and both counts: icpflow_hdbscan_mst; state, keys and values: hdb_pack_kernel for
all n entries (edge slots behind the last edge are not read); labels, keep and the info words: the one upload."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, frame_pairs, utils_cluster, utils_match  # noqa: E402
from test_gpu_cluster_pcd import DEV, OUT_FILL, Guarded, _frame_args, _raw, _synthetic_pair, _two_clouds  # noqa: E402

E_WORKSPACE = -2
POISONS = [pytest.param(0x00, id="p00"), pytest.param(0xA5, id="pA5"), pytest.param(0xFF, id="pFF")]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("hdb", [False, True], ids=["dbscan", "hdbscan"])
def test_cluster_pcd_on_an_exact_poisoned_workspace(hdb, poison):
    pts, a, mask = _two_clouds(hdb)[1]
    cut = len(pts) // 2 + 1
    segs = (pts[:cut], pts[cut:], mask[:cut], mask[cut:])
    ref = _raw(a, *segs)                                       # the ordinary way: the library's cached, larger workspace
    assert int(ref[2][1]) > 0 and int(ref[2][3]) == int(mask.sum())
    for shift in (0, 16):
        got = _raw(a, *segs, poison=poison, shift=shift)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), shift
    rc, untouched = _raw(a, *segs, poison=poison, short=1)
    assert rc == E_WORKSPACE and untouched
    assert b"icpflow_cluster_pcd_workspace_bytes says" in _lib._L.icpflow_last_error()


@pytest.mark.parametrize("cluster", ["dbscan", "hdbscan"])
def test_the_frame_call_refuses_a_short_scratch_with_nothing_written(cluster):
    fp = _synthetic_pair()
    a = _frame_args(cluster, True, 0.8)
    a.translation_frame = frame_pairs.frame_translation(a, fp.pose_exact, 1)
    ps, pd = torch.from_numpy(fp.points_src).to(DEV), torch.from_numpy(fp.points_dst).to(DEV)
    par = utils_cluster.cluster_params(SimpleNamespaceFor(a, cluster))
    reg, keep_alive = utils_match._registration(a, DEV)
    fpar = _lib.FrameParams(ctypes.sizeof(_lib.FrameParams), 0, None, int(a.max_points), int(a.min_cluster_size), float(a.translation_frame),
                            float(a.thres_box), float(a.thres_iou), float(a.thres_rot * 90.0), float(a.thres_error), 1, 1024)
    outs = [Guarded(4 * len(ps), OUT_FILL), Guarded(4 * len(pd), OUT_FILL), Guarded(1024 * 10 * 4, OUT_FILL), Guarded(1024 * 16 * 4, OUT_FILL)]
    pairs, need = ctypes.c_int32(7), ctypes.c_size_t(0)

    def call(scratch, nbytes):
        return _lib._L.icpflow_track_frame_points(_lib.ptr(ps), None, len(ps), _lib.ptr(pd), None, len(pd), ctypes.byref(par),
                                                  _lib.ptr(outs[0].view), _lib.ptr(outs[1].view), ctypes.byref(reg), ctypes.byref(fpar),
                                                  _lib.ptr(outs[2].view), _lib.ptr(outs[3].view), ctypes.byref(pairs), None, None, None,
                                                  scratch, nbytes, ctypes.byref(need), _lib.stream(DEV), None)
    assert call(None, 0) == E_WORKSPACE and need.value > 0
    first = int(need.value)
    cws = int(_lib._L.icpflow_cluster_pcd_workspace_bytes(len(pd), len(ps), ctypes.byref(par)))
    assert first > 256 + cws and first % 256 == 0
    ws = Guarded(first - 1, 0xA5)
    need.value = 0
    assert call(_lib.ptr(ws.view), first - 1) == E_WORKSPACE and need.value == first
    assert b"scratch" in _lib._L.icpflow_last_error()
    torch.cuda.synchronize()
    assert ws.intact() and bool((ws.view == 0xA5).all())
    assert all(o.intact() and bool((o.view == OUT_FILL).all()) for o in outs)
    # ... and the wrapper, which learns the size from such refusals, serves the frame pair
    got = frame_pairs.register_frame_pair_native(a, frame_pairs.make_resident(fp, DEV), DEV)
    assert got is not None and len(got["pairs"]) > 0


def SimpleNamespaceFor(a, cluster):
    from types import SimpleNamespace
    return SimpleNamespace(epsilon=float(a.epsilon), min_cluster_size=int(a.min_cluster_size), num_clusters=int(a.num_clusters),
                           if_hdbscan=cluster == "hdbscan")

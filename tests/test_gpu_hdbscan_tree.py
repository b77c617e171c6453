"""GPU: the HDBSCAN spanning tree (icpflow_hdbscan_mst; csrc/hdbscan.hip) edge for edge beyond ONE group of its chunk walk.

hdbscan.hip sorts the rows by an x-major cell key, cuts them into chunks of 64 and lets a wave walk the chunks outward in
groups of 64 chunks; a direction ends on the running x extreme, chunks uniform in the query's component are skipped unread,
from round 3 on a probe pass over the own group hands the full pass a bound, and the largest component sits a round out.  Up
to 4 096 rows -- all that oracle.hdbscan.mst's dense matrices reach -- there is one group and none of that decides anything.
The scenes of tests/hdbscan_scenes.py have 2 ... 17 groups; their trees come from tests/hdbscan_restatement.py (Prim with
O(n) memory, or the self-certifying tree of the pairs within a radius), pinned to the oracle and to each scene's conditions
by tests/test_hdbscan_restatement.py on the CPU.

EVERYTHING is compared with np.array_equal: n_live, the n_live - 1 edges as (smaller row, larger row) in lexicographic
order (the device appends them in atomic order: test_cluster._gpu_tree's normalisation), their squared weights and the
squared core distances are indices and fp64 numbers computed in a stated operation order; nothing here takes a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import hdbscan_scenes as hs  # noqa: E402
from icp_flow_amd import _lib, utils_cluster  # noqa: E402
from test_cluster import _gpu_tree  # noqa: E402

DEV = torch.device("cuda:0")
POISON = 7.0e8            # what the columns beyond xyz hold in the strided forms


def _normal(a, b, w2):
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    o = np.lexsort((hi, lo))
    return lo[o], hi[o], np.asarray(w2)[o]


def _assert_tree(got, name):
    """got = (lo, hi, w2, core2, n_live) as _gpu_tree returns them, against the scene's restated tree"""
    lo, hi, w2, c2, n_live = got
    rlo, rhi, rw2, rc2 = hs.tree(name)
    rows = hs.live_rows(hs.scene(name))
    assert n_live == len(rows) and len(lo) == len(rows) - 1
    dead = np.ones(len(rc2), bool)
    dead[rows] = False
    assert np.array_equal(c2[rows], rc2[rows]) and np.isnan(c2[dead]).all()
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi), int(((lo != rlo) | (hi != rhi)).sum())
    assert np.array_equal(w2, rw2)


@pytest.mark.parametrize("name", list(hs.SCENES))
def test_tree_equals_the_restatement_edge_for_edge(name):
    sc = hs.scene(name)
    _assert_tree(_gpu_tree(sc.points, sc.k, sc.mask), name)


@pytest.mark.parametrize("name", ["cloud_4200_k2", "slab_8193_far"])
def test_the_cell_only_steers_the_sort(name):
    """0.25 is the product's cell; 0.05 and 8.0 reorder the rows; 1e-4 clamps every coordinate beyond +-104.8 m -- x and y of
    the far slab, whose order is then by z alone -- and spreads the rest over ~10^5 cells per axis; 1e5 puts the whole cloud
    into one cell, so the sorted order is the caller's.  The tree is a function of the points: five times the same arrays."""
    sc = hs.scene(name)
    for cell in (0.25, 0.05, 8.0, 1e-4, 1e5):
        t = utils_cluster.hdbscan_mst(sc.points, sc.k, sc.mask, cell=cell)
        got = (*_normal(t["a"].cpu().numpy(), t["b"].cpu().numpy(), t["w2"].cpu().numpy()), t["core2"].cpu().numpy(), t["n_live"])
        _assert_tree(got, name)


# ------------------------------------------------------------------------------------------------ the raw ABI
def _enqueue(pts, mask, k, cell=0.25, core=True):
    """icpflow_hdbscan_mst on the current stream, on a workspace of exactly the queried size; nothing is read back"""
    n = len(pts)
    need = int(_lib._L.icpflow_hdbscan_mst_workspace_bytes(n))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = dict(core2=torch.full((n,), -7.0, dtype=torch.float64, device=DEV) if core else None,
               a=torch.full((n,), -1, dtype=torch.int32, device=DEV), b=torch.full((n,), -1, dtype=torch.int32, device=DEV),
               w2=torch.full((n,), -7.0, dtype=torch.float64, device=DEV), cnt=torch.full((2,), -1, dtype=torch.int32, device=DEV), ws=ws)
    _lib.call("icpflow_hdbscan_mst", _lib.ptr(pts), pts.shape[1], _lib.ptr(mask), n, int(k), float(cell), _lib.ptr(out["core2"]),
              _lib.ptr(out["a"]), _lib.ptr(out["b"]), _lib.ptr(out["w2"]), _lib.ptr(out["cnt"][0:1]), _lib.ptr(out["cnt"][1:2]),
              _lib.ptr(ws), need, _lib.stream(DEV))
    return out


def _read(out):
    ne, nl = (int(v) for v in out["cnt"].cpu())
    c2 = None if out["core2"] is None else out["core2"].cpu().numpy()
    assert (out["a"][ne:] == -1).all() and (out["w2"][ne:] == -7.0).all()          # nothing written behind the edges
    return (*_normal(out["a"][:ne].cpu().numpy(), out["b"][:ne].cpu().numpy(), out["w2"][:ne].cpu().numpy()), c2, nl)


def _device_form(sc, stride=3):
    p = torch.full((len(sc.points), stride), POISON, dtype=torch.float32, device=DEV)
    p[:, :3] = torch.from_numpy(sc.points).to(DEV)
    if stride > 4:
        p[:, 4] = float("nan")
    m = None if sc.mask is None else torch.from_numpy(sc.mask.astype(np.uint8)).to(DEV)
    return p, m


@pytest.mark.parametrize("name", ["slab_8193_origin", "sparse_4097"])
def test_raw_forms_strides_and_null_pointers(name):
    sc = hs.scene(name)
    for stride in (3, 4, 6):                                  # columns beyond xyz hold 7e8 and NaN: never read
        p, m = _device_form(sc, stride)
        _assert_tree(_read(_enqueue(p, m, sc.k)), name)
    p, m = _device_form(sc)
    lo, hi, w2, c2, nl = _read(_enqueue(p, m, sc.k, core=False))          # d_core2 = NULL: the same edges
    assert c2 is None
    rlo, rhi, rw2, _ = hs.tree(name)
    assert nl == len(hs.live_rows(sc)) and np.array_equal(lo, rlo) and np.array_equal(hi, rhi) and np.array_equal(w2, rw2)
    if sc.mask is None:                                       # d_mask = NULL against a mask of ones (any non-zero byte is on)
        ones = torch.ones(len(p), dtype=torch.uint8, device=DEV)
        ones[::3] = 255
        _assert_tree(_read(_enqueue(p, ones, sc.k)), name)
    else:                                                     # ... and the dead rows dropped by the caller, no mask at all
        fin = np.isfinite(sc.points).all(1)
        q = p.clone()
        q[torch.from_numpy(~sc.mask & fin).to(DEV), 1] = float("inf")      # masked rows made non-finite instead
        _assert_tree(_read(_enqueue(q, None, sc.k)), name)


@pytest.mark.parametrize("k", [1, 2])
def test_one_live_row_among_300(k):
    """no edge; the row's core distance is 0 for k = 1 and +inf (no k-th neighbour) beyond; NaN on the other rows"""
    p = np.random.default_rng(8).random((300, 3)).astype(np.float32)
    mask = np.zeros(300, np.uint8)
    mask[211] = 1
    p[5, 2] = np.nan
    lo, hi, w2, c2, nl = _read(_enqueue(torch.from_numpy(p).to(DEV), torch.from_numpy(mask).to(DEV), k))
    assert nl == 1 and len(lo) == 0
    assert c2[211] == (0.0 if k == 1 else np.inf) and np.isnan(np.delete(c2, 211)).all()
    if k == 1:
        t = utils_cluster.hdbscan_mst(p, 1, mask.astype(bool))
        assert t["n_live"] == 1 and t["a"].numel() == 0
    else:
        with pytest.raises(ValueError):
            utils_cluster.hdbscan_mst(p, 2, mask.astype(bool))


def test_reruns_and_two_streams_at_once_give_identical_output():
    name = "slab_8900_far"
    sc = hs.scene(name)
    p, m = _device_form(sc)
    for _ in range(3):
        _assert_tree(_read(_enqueue(p, m, sc.k)), name)
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s in sides:                                           # both enqueued before either is waited for
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(_enqueue(p, m, sc.k))
    for s in sides:
        s.synchronize()
    for out in outs:
        _assert_tree(_read(out), name)


def test_labels_from_the_gpu_tree_equal_labels_from_the_restated_tree():
    """the host half (icpflow_hdbscan_labels) sees a tree of three groups: hdbscan()'s labels = labels_from_mst on the
    restated tree, and the clusters are not trivial"""
    name = "sparse_8193"
    sc = hs.scene(name)
    lo, hi, w2, _ = hs.tree(name)
    rows = hs.live_rows(sc)
    sub = np.full(len(sc.points), -1, np.int64)
    sub[rows] = np.arange(len(rows))
    mcs = 12
    want = utils_cluster.labels_from_mst(sub[lo], sub[hi], np.sqrt(w2), len(rows), mcs)
    got = utils_cluster.hdbscan(sc.points, mcs, min_samples=sc.k, mask=sc.mask, counts_self=True)
    fin = np.isfinite(sc.points).all(1)
    assert np.array_equal(got[rows], want) and (got[~sc.mask] == -2).all() and (got[sc.mask & ~fin] == -1).all()
    assert want.max() >= 1 and (want < 0).any()

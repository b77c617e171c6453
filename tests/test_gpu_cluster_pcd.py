"""GPU: cluster_pcd behind the C ABI (icpflow_cluster_pcd, icpflow_track_frame_points; csrc/clusterpcd.hip).

Every label is compared with `torch.equal` against the existing Python path (utils_cluster.cluster_pcd without the switch) on
the same inputs.  numpy's tie order at the cut is not the library's (the named deviation): wherever the two are compared the
test reads the cluster sizes back and asserts that no tie in size straddles the cut; the tie rule itself has a test of its own,
against the named rule."""
import ctypes
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, frame_pairs, synthetic, utils_cluster  # noqa: E402

DEV = torch.device("cuda:0")
GUARD, GUARD_BYTE, OUT_FILL = 1 << 20, 0x3C, 0x6B


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _args(eps=0.25, mcs=3, ncl=5, hdb=False, **over):
    return SimpleNamespace(epsilon=float(eps), min_cluster_size=int(mcs), num_clusters=int(ncl), if_hdbscan=hdb, **over)


def _sizes(a, pts, mask):
    """(cluster sizes, noise rows) as the existing path sees them, read back."""
    if a.if_hdbscan:
        raw = utils_cluster.hdbscan(pts, a.min_cluster_size, None, mask)
        return np.bincount(raw[raw >= 0], minlength=0), int((raw == -1).sum())
    lab, sizes = utils_cluster.dbscan(pts, a.epsilon, a.min_cluster_size, mask)
    return sizes.cpu().numpy(), int((lab == -1).sum())


def assert_cut_is_tie_free(a, pts, mask):
    sizes, noise = _sizes(a, pts, mask)
    s = np.sort(sizes[0 if noise > 0 else 1:])[::-1]
    assert not (a.num_clusters < len(s) and s[a.num_clusters - 1] == s[a.num_clusters]), ("a tie in size straddles the cut", a.num_clusters)
    return sizes, noise


def both_paths(a, pts, mask, n_dst=None):
    """-> labels float64 [n] of the native call, after comparing them with the existing path; the stack is split at n_dst."""
    n = len(pts)
    n_dst = n if n_dst is None else n_dst
    assert_cut_is_tie_free(a, pts, mask)
    want = utils_cluster.cluster_pcd(a, pts, mask)
    src, msrc = (pts[n_dst:], mask[n_dst:]) if n_dst < n else (None, None)
    ld, ls = utils_cluster.cluster_pcd_native(a, pts[:n_dst], src, mask[:n_dst], msrc)
    got = ld if ls is None else torch.cat([ld, ls])
    assert got.dtype == torch.float32 and want.dtype == torch.float64
    assert torch.equal(got.double(), want)
    # ... and through the switch of cluster_pcd itself
    a2 = SimpleNamespace(**vars(a), native_cluster=True)
    via = utils_cluster.cluster_pcd(a2, pts, mask)
    assert via.dtype == torch.float64 and torch.equal(via, want)
    return want


# ------------------------------------------------------------------------------------------ DBSCAN
@pytest.mark.parametrize("k", [0, 1, 2])
def test_dbscan_small_clouds(k):
    g = load_golden("g10_dbscan")
    p, ng, want = g[f"small_{k}_points"], g[f"small_{k}_nonground"], g[f"small_{k}_labels"]
    eps, mcs, ncl = g[f"small_{k}_params"]
    got = both_paths(_args(eps, mcs, ncl), G(p), G(ng), n_dst=len(p) // 3)
    assert np.array_equal(got.cpu().numpy(), want)      # G10: the reference's own run


def blob_lattice(C, noise_rows, seed=0):
    """C blobs of 2 to 9 points on a lattice 5 m apart (eps 0.25, min_points 2: every blob is one cluster, ids in blob order), one
    blob of 2 and one of 9 points so that the cuts at 1 and at C - 1 are tie-free, `noise_rows` single points.  -> points [n,3]"""
    rng = np.random.default_rng(seed + C)
    sizes = rng.integers(3, 9, size=C)
    if C >= 1:
        sizes[(2 * C) // 3] = 9
    if C >= 2:
        sizes[C // 3] = 2
    rows = []
    for k, s in enumerate(list(sizes) + [1] * noise_rows):
        base = np.array([(k % 40) * 5.0, (k // 40) * 5.0, 0.0])
        rows.append(base + np.arange(s)[:, None] * np.array([0.01, 0.0, 0.0]))
    return np.concatenate(rows).astype(np.float32), sizes


@pytest.mark.parametrize("C", [0, 1, 2, 255, 256, 257, 1025])
def test_dbscan_blob_lattices_cover_the_rank_kernels_borders(C):
    """Exactly C clusters in a few thousand points: the tile (256 sizes in LDS) and workgroup borders of the keep-rule kernel;
    num_clusters = C - 1, C, C + 1 and 1."""
    p, sizes = blob_lattice(C, noise_rows=7)
    pts, mask = G(p), torch.ones(len(p), dtype=torch.bool, device=DEV)
    for ncl in sorted({max(C - 1, 1), max(C, 1), C + 1, 1}):
        a = _args(0.25, 2, ncl)
        if C == 0:                                # nothing to keep: both paths raise as upstream
            for fn in (lambda: utils_cluster.cluster_pcd(a, pts, mask), lambda: utils_cluster.cluster_pcd_native(a, pts, None, mask, None)):
                with pytest.raises(IndexError):
                    fn()
            ld, _ = utils_cluster.cluster_pcd_native(a, pts, None, mask, None, check=False)
            assert bool((ld == -1).all())
            continue
        got = both_paths(a, pts, mask, n_dst=len(p) // 2).cpu().numpy()
        kept = np.unique(got[got >= 0]).astype(np.int64)
        assert len(kept) == min(ncl, C)
        if ncl == 1:
            assert kept.tolist() == [(2 * C) // 3]
        if ncl == C - 1:
            assert C // 3 not in kept


def blobs(sizes):
    """One blob of s points per entry, 5 m apart: cluster k has sizes[k] rows (eps 0.25, min_points 2); an entry of 1 is a noise row."""
    rows = [np.array([k * 5.0, 0.0, 0.0]) + np.arange(s)[:, None] * np.array([0.01, 0.0, 0.0]) for k, s in enumerate(sizes)]
    return G(np.concatenate(rows).astype(np.float32))


def test_dbscan_without_a_noise_row_cluster_zero_is_never_kept():
    """No row is noise: np.unique's first label, dropped unseen, is cluster 0 -- the largest cluster here."""
    pts = blobs([9, 5, 3, 7, 4, 6])
    mask = torch.ones(len(pts), dtype=torch.bool, device=DEV)
    for ncl in (1, 4, 5, 6, 200):
        got = both_paths(_args(0.25, 2, ncl), pts, mask).cpu().numpy()
        assert (got[:9] == -1).all()                                  # every row of cluster 0 reads -1
        assert len(np.unique(got[got >= 0])) == min(ncl, 5)
    assert np.unique(both_paths(_args(0.25, 2, 1), pts, mask).cpu().numpy()).tolist() == [-1.0, 3.0]
    assert _raw(_args(0.25, 2, 200), pts, None, mask, None)[2].tolist() == [6, 5, 0, len(pts)]


def test_dbscan_masks_segments_and_one_cloud():
    pts = blobs([12, 3, 15, 6, 9, 18, 21, 24, 1, 1])     # (sizes that stay distinct at the cut of 4 under the mask below)
    n = len(pts)
    a = _args(0.25, 2, 4)
    none = torch.zeros(n, dtype=torch.bool, device=DEV)
    # all rows masked: nothing is clustered, the reference's expression has nothing to sort
    for fn in (lambda: utils_cluster.cluster_pcd(a, pts, none), lambda: utils_cluster.cluster_pcd_native(a, pts, None, none, None)):
        with pytest.raises(IndexError):
            fn()
    ld, ls, info = _raw(a, pts[:5], pts[5:], none[:5], none[5:])
    assert bool((ld == -1e8).all()) and bool((ls == -1e8).all()) and info.tolist() == [0, 0, 0, 0]
    one = none.clone()
    one[7] = True
    ld, ls, info = _raw(a, pts[:5], pts[5:], one[:5], one[5:])
    assert info.tolist() == [0, 0, 1, 1] and float(ls[2]) == -1.0 and int((torch.cat([ld, ls]) == -1e8).sum()) == n - 1
    # a real mask; segment lengths 1 and 63 / 64 / 65; n_src = 0; no mask pointer at all = a mask of ones
    mask = torch.ones(n, dtype=torch.bool, device=DEV)
    mask[::7] = False
    want = None
    for n_dst in (1, 63, 64, 65, n - 1, n):
        got = both_paths(a, pts, mask, n_dst=n_dst)
        assert want is None or torch.equal(got, want)
        want = got
    ones = torch.ones(n, dtype=torch.bool, device=DEV)
    ld, ls, _ = _raw(a, pts[:64], pts[64:], None, None)
    assert torch.equal(torch.cat([ld, ls]).double(), both_paths(a, pts, ones))
    # a stride of 4 floats (x, y, z, flag) reads the same points
    p4 = torch.cat([pts, torch.full((n, 1), 7.0, device=DEV)], dim=1).contiguous()
    ld4, ls4, _ = _raw(a, p4[:64], p4[64:], None, None)
    assert torch.equal(ld4, ld) and torch.equal(ls4, ls)


def test_dbscan_tie_at_the_cut_follows_the_named_rule():
    """Four blobs of sizes 4, 4, 4, 9 and a noise row, num_clusters = 2: among the equal sizes the LARGER id survives (asserted
    against the library's named rule; numpy's unstable argsort promises nothing here)."""
    pts = blobs([4, 4, 4, 9, 1])
    ld, _, info = _raw(_args(0.25, 2, 2), pts, None, None, None)
    assert ld.tolist() == [-1.0] * 8 + [2.0] * 4 + [3.0] * 9 + [-1.0] and info.tolist() == [4, 2, 1, 22]
    ld, _, info = _raw(_args(0.25, 2, 3), pts, None, None, None)
    assert ld.tolist() == [-1.0] * 4 + [1.0] * 4 + [2.0] * 4 + [3.0] * 9 + [-1.0] and info.tolist() == [4, 3, 1, 22]


def _demo():
    g = load_golden("g8_demo")
    return g["point_dst"], g["point_src"]


def test_dbscan_demo_frame():
    g = load_golden("g10_dbscan")
    dst, src = _demo()
    pts = G(np.concatenate([dst, src]))
    eps, mcs, ncl = g["demo_a_params"]
    got = both_paths(_args(eps, mcs, ncl), pts, torch.ones(len(pts), dtype=torch.bool, device=DEV), n_dst=len(dst))
    assert np.array_equal(got.cpu().numpy().astype(np.int32), g["demo_a_labels"])


# ------------------------------------------------------------------------------------------ HDBSCAN
@pytest.mark.parametrize("case", ["crop_0", "crop_1", "nonfinite", "synth"])
def test_hdbscan_small_clouds(case):
    g = load_golden("g11_hdbscan")
    src = "crop_2" if case == "nonfinite" else case
    p, (k, ncl) = g[f"{src}_points"].copy(), g[f"{src}_params"]
    mask = g["synth_nonground"].copy() if case == "synth" else np.ones(len(p), dtype=bool)
    if case == "nonfinite":
        p[5] = np.nan
        p[len(p) // 2, 1] = np.inf
        p[-1, 2] = -np.inf
    a = _args(0.25, int(k), int(ncl), hdb=True)
    got = both_paths(a, G(p), G(mask), n_dst=len(p) // 2).cpu().numpy()
    assert (got[~mask] == -1e8).all() and (got[mask] >= -1).all()
    if case == "nonfinite":
        assert got[5] == -1 and got[len(p) // 2] == -1 and got[-1] == -1
    # too few points for min_samples: refused with a message (the hdbscan package raises there as well)
    if case == "crop_0":
        with pytest.raises(RuntimeError, match="cannot be clustered"):
            utils_cluster.cluster_pcd_native(a, G(p[:int(k)]), None, None, None)


def test_hdbscan_demo_frame():
    dst, src = _demo()
    pts = G(np.concatenate([dst, src]))
    a = _args(0.25, 20, 200, hdb=True)                      # G11's settings
    got = both_paths(a, pts, torch.ones(len(pts), dtype=torch.bool, device=DEV), n_dst=len(dst))
    assert int(got.max()) > 100


# ------------------------------------------------------------------------------------------ both branches, the C caller's way
class Guarded:
    """[front guard | nbytes | back guard] in one allocation; `.view` is the exact-size middle, 256-aligned (+ shift)."""

    def __init__(self, nbytes, fill, shift=0):
        self.raw = torch.full((GUARD + 256 + shift + int(nbytes) + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        base = self.raw.data_ptr()
        self.start = (base + GUARD + 255) // 256 * 256 - base + shift
        self.view = self.raw[self.start:self.start + int(nbytes)]
        self.view.fill_(fill)

    def intact(self):
        torch.cuda.synchronize()
        end = self.start + self.view.numel()
        return bool((self.raw[:self.start] == GUARD_BYTE).all()) and bool((self.raw[end:] == GUARD_BYTE).all())


def _raw(a, dst, src, mdst, msrc, poison=None, shift=0, short=0, stream=None):
    """icpflow_cluster_pcd the way a C caller runs it: outputs and d_info between guard bytes; with `poison` the workspace too, at
    exactly the size the query names (minus `short`).  -> (labels_dst, labels_src, info) or, with short, (status, all untouched)."""
    par = utils_cluster.cluster_params(a)
    nd, ns = len(dst), 0 if src is None else len(src)
    dst = dst.float().contiguous()
    src = None if src is None else src.float().contiguous()
    u8 = lambda m: None if m is None else m.to(torch.uint8).contiguous()   # noqa: E731
    mdst, msrc = u8(mdst), u8(msrc)
    need = int(_lib._L.icpflow_cluster_pcd_workspace_bytes(nd, ns, ctypes.byref(par)))
    assert need > 0 and need % 256 == 0
    outs = [Guarded(4 * nd, OUT_FILL), Guarded(4 * ns, OUT_FILL), Guarded(16, OUT_FILL)]
    ws = Guarded(need, poison, shift) if poison is not None else None
    ws_t = ws.view if ws is not None else _lib.workspace(DEV, need)
    ws_bytes = need - short if ws is not None else ws_t.numel()
    rc = _lib._L.icpflow_cluster_pcd(_lib.ptr(dst), nd, _lib.ptr(src), ns, dst.shape[1], _lib.ptr(mdst), _lib.ptr(msrc), ctypes.byref(par),
                                     _lib.ptr(outs[0].view) if nd else None, _lib.ptr(outs[1].view) if ns else None, _lib.ptr(outs[2].view),
                                     _lib.ptr(ws_t), ws_bytes, ctypes.c_void_p(stream) if stream else _lib.stream(DEV))
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and (ws is None or ws.intact()), "guard bytes changed"
    if short:
        return rc, all(bool((o.view == OUT_FILL).all()) for o in outs) and bool((ws.view == poison).all())
    assert rc == 0, (rc, _lib._L.icpflow_last_error())
    return outs[0].view.view(torch.float32).clone(), outs[1].view.view(torch.float32).clone(), outs[2].view.view(torch.int32).cpu()


def _two_clouds(hdb):
    """-> two of (points, args, mask): for DBSCAN lattices of 300 and 257 blobs cut at C - 1 (tie-free: one smallest blob), the
    mask taking noise rows only; for HDBSCAN two of G11's crops, every eleventh row masked."""
    out = []
    for k in (0, 1):
        if hdb:
            g = load_golden("g11_hdbscan")
            pts = G(g[f"crop_{k}_points"])
            a = _args(0.25, int(g[f"crop_{k}_params"][0]), int(g[f"crop_{k}_params"][1]), hdb=True)
            mask = torch.ones(len(pts), dtype=torch.bool, device=DEV)
            mask[3::11] = False
        else:
            C = (300, 257)[k]
            pts = G(blob_lattice(C, 5)[0])
            a = _args(0.25, 2, C - 1)
            mask = torch.ones(len(pts), dtype=torch.bool, device=DEV)
            mask[-3:] = False
        out.append((pts, a, mask))
    return out


@pytest.mark.parametrize("hdb", [False, True], ids=["dbscan", "hdbscan"])
def test_guards_poisoned_workspace_and_reruns(hdb):
    pts, a, mask = _two_clouds(hdb)[0]
    n = len(pts)
    want = both_paths(a, pts, mask, n_dst=n // 3)
    ref = _raw(a, pts[:n // 3], pts[n // 3:], mask[:n // 3], mask[n // 3:])
    assert torch.equal(torch.cat(ref[:2]).double(), want)
    sizes, noise = _sizes(a, pts, mask)
    first = 0 if noise > 0 else 1
    assert ref[2].tolist() == [len(sizes), min(a.num_clusters, len(sizes) - first), noise, int(mask.sum())]
    for poison, shift in ((0x00, 0), (0xA5, 0), (0xFF, 0), (0xFF, 16)):
        got = _raw(a, pts[:n // 3], pts[n // 3:], mask[:n // 3], mask[n // 3:], poison=poison, shift=shift)
        for x, y in zip(got, ref):                       # bit-identical reruns, whatever the scratch held
            assert torch.equal(x, y), (poison, shift)


@pytest.mark.parametrize("hdb", [False, True], ids=["dbscan", "hdbscan"])
def test_two_streams_at_once(hdb):
    """Two clouds clustered at once, a host thread and a stream each (the HDBSCAN branch blocks its caller): what each gets
    alone."""
    clouds = _two_clouds(hdb)
    alone = [utils_cluster.cluster_pcd_native(a, p[:100], p[100:], m[:100], m[100:]) for p, a, m in clouds]
    torch.cuda.synchronize()
    out, errors = [None, None], []

    def work(k):
        try:
            torch.cuda.set_device(DEV)
            with torch.cuda.stream(torch.cuda.Stream(DEV)):
                for _ in range(3):
                    p, a, m = clouds[k]
                    out[k] = utils_cluster.cluster_pcd_native(a, p[:100], p[100:], m[:100], m[100:])
                torch.cuda.current_stream().synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for got, want in zip(out, alone):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------ icpflow_track_frame_points
def _frame_args(cluster, native, epsilon=0.25):
    a = frame_pairs.default_args(max_points=2048, cluster=cluster, epsilon=epsilon, min_cluster_size=20, num_clusters=200)
    a.if_verbose = True
    if native:
        a.native_cluster = True
    return a


def _synthetic_pair(seed=5):
    d = synthetic.make_frame_pair(seed=seed, n_objects=8, n_min=200, n_max=1500, n_background=1500)
    return frame_pairs.FramePair(d["points_src"], d["points_dst"], None, None, d["pose"], d["gt_flow"],
                                 nonground_src=d["labels_src"] > -1e7, nonground_dst=d["labels_dst"] > -1e7)


def _demo_pair():
    g = load_golden("g8_demo")
    return frame_pairs.FramePair(g["point_src"], g["point_dst"], None, None, None, g["gt_flow"])


def _same_result(got, want):
    assert got is not None and want is not None and got is not frame_pairs.NEEDS_HOST_ASSOCIATION
    for key in ("pairs", "transformations", "flow", "labels_src", "labels_dst"):
        assert torch.equal(got[key], want[key]), key
    assert len(got["pairs"]) > 0


@pytest.mark.parametrize("cluster", ["dbscan", "hdbscan"])
@pytest.mark.parametrize("which", ["synthetic", "demo"])
def test_frame_from_points_equals_clustering_then_track_frame(which, cluster):
    """icpflow_track_frame_points against the existing Python clustering followed by icpflow_track_frame: pairs, transforms,
    flow and the labels handed back, bit for bit."""
    fp = frame_pairs.make_resident(_synthetic_pair() if which == "synthetic" else _demo_pair(), DEV)
    ps, pd = G(fp.points_src), G(fp.points_dst)
    m = lambda x, n: torch.ones(n, dtype=torch.bool, device=DEV) if x is None else G(x)   # noqa: E731
    eps = 0.8 if which == "synthetic" else 0.25          # (the synthetic shells are sparser than a LiDAR frame)
    assert_cut_is_tie_free(_args(eps, 20, 200, hdb=cluster == "hdbscan"), torch.cat([pd, ps]),
                           torch.cat([m(fp.nonground_dst, len(pd)), m(fp.nonground_src, len(ps))]))
    want = frame_pairs.register_frame_pair_native(_frame_args(cluster, False, eps), fp, DEV)
    got = frame_pairs.register_frame_pair_native(_frame_args(cluster, True, eps), fp, DEV)
    _same_result(got, want)


def test_four_frame_pairs_in_flight_equal_one_after_the_other():
    fps = [frame_pairs.make_resident(_synthetic_pair(seed), DEV) for seed in (5, 6, 7, 8)]
    a = _frame_args("dbscan", True, 0.8)
    one = [frame_pairs.register_frame_pair_native(a, fp, DEV) for fp in fps]
    seen = 0
    for k, _, got in frame_pairs.register_in_flight_native(a, fps, DEV, in_flight=4):
        _same_result(got, one[k])
        seen += 1
    assert seen == 4


def test_run_sequences_meters_equal_with_and_without_the_switch(tmp_path):
    import os
    d = synthetic.make_sequence(seed=3, num_frames=3, n_objects=6, n_max=400)
    sd = (d["nonground"] & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    os.makedirs(os.path.join(tmp_path, "val"))
    path = os.path.join(tmp_path, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=d["nonground"].astype(np.int64))
    res = []
    for native in (False, True):
        a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
        a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.05, False, "ego_motion_gt"
        if native:
            a.native_cluster = True
        res.append(frame_pairs.run_sequences(a, [path], DEV))
    assert res[0]["frame_pairs"] == res[1]["frame_pairs"] == 2
    for name, want in res[0]["metrics"].items():
        got = res[1]["metrics"][name]
        assert vars(got).keys() == vars(want).keys()
        for key, v in vars(want).items():
            assert np.array_equal(np.asarray(v, dtype=np.float64), np.asarray(vars(got)[key], dtype=np.float64), equal_nan=True), (name, key)

"""CPU-only tests of the ground segmentation: the new entry points of the C ABI answer argument errors with status codes, the
Python functions refuse to run without a GPU, `--ground auto` is what `_sequence_ground` did before, and the fp64 restatement
(tests/ground_restatement.py) the GPU tests hold the kernels against does what the method says on scenes one can reason about
-- with every scene of tests/ground_scenes.py clear of the method's thresholds (at most 1 % of its patches undetermined)."""
import ctypes
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_restatement as gr      # noqa: E402
import ground_scenes as gs           # noqa: E402


@functools.lru_cache(maxsize=None)
def scene(name):
    pts, parts = gs.ALL[name]()
    return pts, parts, gr.segment(pts)


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    from icp_flow_amd import _lib
    L, one = _lib._L, ctypes.c_void_p(256)
    assert L.icpflow_ground_default_params(None) == -1 and b"null pointer" in L.icpflow_last_error()
    par = _lib.GroundParams.defaults()
    assert par.struct_size == ctypes.sizeof(_lib.GroundParams) == 128
    assert (par.sensor_height, par.min_range, par.max_range, par.num_iter, par.num_lpr, par.num_min_pts) == (1.723, 1.0, 64.0, 3, 20, 10)
    assert (par.th_seeds, par.th_dist, par.th_seeds_v, par.th_dist_v, par.uprightness_thr) == (0.125, 0.125, 0.25, 0.1, 0.707)
    assert par.adaptive_seed_selection_margin == -1.2 and par.num_rings_of_interest == 4
    assert list(par.num_sectors_each_zone) == [16, 32, 54, 32] and list(par.num_rings_each_zone) == [2, 4, 4, 4]
    ref = ctypes.byref(par)
    seg = lambda pts, stride, n, p, out, ws, nbytes: L.icpflow_ground_segment(pts, stride, n, p, out, None, ws, ctypes.c_size_t(nbytes), None)   # noqa: E731
    need = L.icpflow_ground_workspace_bytes(3000, ref)
    assert need > 3000 * 21 and need % 256 == 0 and L.icpflow_ground_workspace_bytes(0, ref) == 0
    sizes = [L.icpflow_ground_workspace_bytes(n, ref) for n in (1, 9, 512, 513, 3000, 20000, 120000, 1 << 20, (1 << 31) - 1)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    assert seg(one, 3, 100, None, one, one, need) == -1 and b"null pointer" in L.icpflow_last_error()
    assert seg(None, 3, 100, ref, one, one, need) == -1 and b"null pointer" in L.icpflow_last_error()
    assert seg(one, 3, 100, ref, None, one, need) == -1 and b"null pointer" in L.icpflow_last_error()
    assert seg(one, 2, 100, ref, one, one, need) == -1 and b"stride" in L.icpflow_last_error()
    assert seg(one, 3, -1, ref, one, one, need) == -1
    assert seg(one, 3, 3000, ref, one, one, need - 1) == -2 and b"workspace" in L.icpflow_last_error()
    assert seg(one, 3, 3000, ref, one, None, need) == -2 and b"workspace" in L.icpflow_last_error()
    assert seg(one, 3, 3000, ref, one, ctypes.c_void_p(260), need) == -1 and b"aligned" in L.icpflow_last_error()
    assert seg(None, 3, 0, ref, None, None, 0) == 0                       # n == 0: a success that writes nothing
    bad = _lib.GroundParams.defaults()
    bad.struct_size -= 8
    assert seg(one, 3, 100, ctypes.byref(bad), one, one, need) == -1 and b"struct_size" in L.icpflow_last_error()
    assert L.icpflow_ground_workspace_bytes(100, ctypes.byref(bad)) == 0
    for field, k, v in (("num_sectors_each_zone", 2, 48), ("num_rings_each_zone", 0, 4), ("num_rings_of_interest", None, 3)):
        bad = _lib.GroundParams.defaults()
        if k is None:
            setattr(bad, field, v)
        else:
            getattr(bad, field)[k] = v
        assert seg(one, 3, 100, ctypes.byref(bad), one, one, need) == -1 and b"zone layout" in L.icpflow_last_error()


def test_there_is_no_cpu_path():
    from icp_flow_amd import utils_ground
    a = SimpleNamespace(range_z=0.0, ground_slack=0.3)
    x = torch.zeros(20, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_ground.segment_ground_pypatchworkpp(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_ground.segment_ground(a, x)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            utils_ground.segment_ground(a, np.zeros((20, 3)))
    assert utils_ground.segment_ground_thres(a, np.array([[0, 0, 0.2], [0, 0, 0.4]])).tolist() == [False, True]


def test_ground_auto_is_what_sequence_ground_did():
    from icp_flow_amd import frame_pairs, utils_ground
    rng = np.random.default_rng(0)
    raw, t = rng.normal(size=(50, 3)), np.repeat(np.arange(5), 10)
    fps = lambda: [SimpleNamespace(gap=j, nonground_src=None, nonground_dst=None) for j in range(1, 5)]   # noqa: E731
    for extra in ({}, {"ground": "auto"}):
        a = SimpleNamespace(range_z=0.0, ground_slack=0.3, **extra)
        f = fps()
        assert frame_pairs._sequence_ground(a, dict(nonground=np.ones(50, bool), raw_points=raw, time_indice=t), f) == "nonground key"
        assert all(fp.nonground_src is None for fp in f)
        assert frame_pairs._sequence_ground(a, dict(nonground=None, raw_points=raw, time_indice=t), f) == "threshold"
        ng = utils_ground.segment_ground_thres(a, raw)
        assert all((fp.nonground_src == ng[t == fp.gap]).all() and (fp.nonground_dst == ng[t == 0]).all() for fp in f)
        assert frame_pairs._sequence_ground(SimpleNamespace(**extra), dict(nonground=None, raw_points=raw, time_indice=t), fps()) == "none"
    with pytest.raises(ValueError, match="range_z"):
        frame_pairs._sequence_ground(SimpleNamespace(ground="patchwork"), dict(nonground=None, raw_points=raw, time_indice=t), fps())


def test_binning_edges_of_the_restatement():
    pts, parts, res = scene("edges")
    sp = parts["special"]
    pid = res["patch"][sp]
    xy = pts[sp, 0:2]
    on = lambda x, y: int(pid[np.flatnonzero((xy[:, 0] == np.float32(x)) & (xy[:, 1] == np.float32(y)))[0]])   # noqa: E731
    assert on(1, 0) == -1 and on(0, 1) == -1 and on(0.5, 0.5) == -1 and on(100, 3) == -1 and on(0, 0) == -1
    assert on(64, 0) == gr.patch_index(3, 3, 31) and on(0, -64) == gr.patch_index(3, 3, 24) and on(63, 1e-3) == gr.patch_index(3, 3, 0)
    for zone, b in enumerate(gr.LO[1:], start=1):                          # a boundary belongs to the outer zone
        assert on(b, 0) == gr.patch_index(zone, 0, gr.SECTORS[zone] - 1) and on(-b, 0) == gr.patch_index(zone, 0, gr.SECTORS[zone] // 2)
    assert (pid[-5:] == -1).all()                                          # NaN / inf rows
    # y = +-0 with x > 0: the last sector; x < 0: the middle one
    rows = {(float(x), float(np.copysign(1, y))): int(p) for (x, y), p in zip(xy, pid)}
    assert rows[(5.0, 1.0)] == rows[(5.0, -1.0)] == gr.patch_index(0, 1, 15)
    assert rows[(-5.0, 1.0)] == rows[(-5.0, -1.0)] == gr.patch_index(0, 1, 8)
    assert rows[(20.0, 1.0)] == rows[(20.0, -1.0)] == gr.patch_index(2, 0, 53) and rows[(40.0, -1.0)] == gr.patch_index(3, 0, 31)
    assert res["nonground"][parts["nine"]].all() and not res["nonground"][parts["ten"]].any()
    assert not res["nonground"][parts["last_sector"]].any() and res["table"][15, 0] == 30


def test_restatement_on_flat_ground_under_boxes():
    pts, parts, res = scene("flat_boxes")
    assert not res["nonground"][parts["ground"]].any()
    up = parts["boxes"][pts[parts["boxes"], 2] > -1.4]
    assert len(up) > 100 and res["nonground"][up].all()


def test_restatement_removes_a_wall_in_zone_0_only():
    pts, parts, res = scene("walls")
    t, p0, p1 = res["table"], gr.patch_index(0, 0, 2), gr.patch_index(1, 1, 9)
    assert t[p0, 14] >= 400 and res["nonground"][parts["wall0"]].all() and not res["nonground"][parts["ground0"]].all()
    assert t[p1, 14] == 0 and t[gr.patch_index(0, 1, 5), 14] == 300 and t[gr.patch_index(0, 1, 5), 1] == 0
    assert np.isnan(t[gr.patch_index(1, 2, 4), 5:12]).all() and res["nonground"][parts["outlier"]].all()
    assert t[gr.patch_index(2, 1, 10), 12] == gr.FAR and t[gr.patch_index(2, 1, 30), 12] == gr.NOT_UPRIGHT
    assert not res["nonground"][parts["all_below"]].any()


def test_restatement_reverts_by_ring():
    pts, parts, res = scene("platform")
    t = res["table"]
    code = lambda z, r, s: (int(t[gr.patch_index(z, r, s), 12]), int(t[gr.patch_index(z, r, s), 13]))   # noqa: E731
    assert code(0, 1, 6) == (gr.CANDIDATE, gr.TGR_REVERTED) and code(0, 1, 8) == (gr.CANDIDATE, gr.TGR_REJECTED)
    assert code(0, 1, 10) == (gr.CANDIDATE, gr.TGR_REVERTED) and t[gr.patch_index(0, 1, 10), 1] > 1500
    assert code(0, 1, 12) == (gr.CANDIDATE, gr.TGR_REJECTED) and t[gr.patch_index(0, 1, 12), 8] / t[gr.patch_index(0, 1, 12), 9] > 8
    assert code(1, 1, 17) == (gr.CANDIDATE, gr.TGR_REJECTED)               # one listed value: mu = 0
    assert not res["nonground"][parts["smooth"]].any() and res["nonground"][parts["rough"]].all()


def test_restatement_carries_the_flatness_list_over_a_ring_without_candidates():
    """Ring 0 of `platform` has no candidates, so its flatness values are still listed when ring 1 is judged, and they decide
    `middle`: reverted with the carried list, rejected by what ring 1's own values would give -- and not by a margin a rounding
    could close."""
    pts, parts, res = scene("platform")
    t, q = res["table"], gr.patch_index(0, 1, 14)
    assert 0 not in res["rings"] and sorted(res["rings"]) == [1, 3]
    ring = res["rings"][1]
    assert len(ring["own"]) == 4 and len(ring["listed"]) == 8 + 4 and ring["listed"][8:] == ring["own"]

    def prob(values, f):
        v = np.float64(values)
        mu = v.mean() + 1.5 * v.std(ddof=1)
        return mu, 1.0 / (1.0 + np.exp((f - mu) / (mu / 10.0)))

    f = t[q, 10]
    (mu_carried, p_carried), (mu_own, p_own) = prob(ring["listed"], f), prob(ring["own"], f)
    print(f"flatness {f:.3e}: mu {mu_carried:.3e} -> p {p_carried:.3f} with ring 0's values, mu {mu_own:.3e} -> p {p_own:.3f} without")
    assert abs(mu_carried - ring["mu"]) <= 1e-12 * mu_carried
    assert t[q, 8] / t[q, 9] < 8 and t[q, 1] <= 1500                     # neither the line test nor the count decides it
    assert p_carried > 0.9 and p_own < 0.1
    assert (int(t[q, 12]), int(t[q, 13])) == (gr.CANDIDATE, gr.TGR_REVERTED) and not res["nonground"][parts["middle"]].all()
    # the other candidates of the ring fall the same way under either mu, so `middle` alone shows the rule
    assert gr.determined(res)[q]


def test_rows_are_clear_of_the_borders_of_the_binning():
    """Every row of every scene is at least 1e-9 of a bin away from a ring or sector border, except the rows `edges` puts on
    one on purpose (ground_restatement.border_distance says why those are exact)."""
    for name in sorted(gs.ALL):
        pts, parts, res = scene(name)
        rows = np.ones(len(pts), dtype=bool)
        if name == "edges":
            rows[parts["special"]] = False
            assert (res["border"][parts["special"]] < 1e-6).sum() >= 20     # the scene is on the borders
        print(name, "smallest distance to a border, in bins:", res["border"][rows].min())
        assert res["border"][rows].min() > 1e-9


@pytest.mark.parametrize("name", sorted(gs.ALL))
def test_scene_is_clear_of_the_thresholds(name):
    _, _, res = scene(name)
    big = res["table"][:, 0] >= gr.NUM_MIN_PTS
    und = big & ~gr.determined(res)
    print(name, "patches of >= 10 points:", int(big.sum()), "undetermined:", int(und.sum()))
    assert big.sum() >= 3 and und.sum() <= 0.01 * big.sum()


def test_default_params_are_bit_for_bit_what_the_module_constants_gave():
    """segment(pts) without params on two existing scenes against the values from before it took any, kept in tests/golden"""
    import ground_scenes as gs
    before = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ground_restatement_before_params.npz"))
    for name in ("walls", "platform"):
        pts, _ = gs.ALL[name]()
        for res in (gr.segment(pts), gr.segment(pts, gr.Params())):
            for k in ("nonground", "table", "margin", "gap"):
                assert res[k].tobytes() == before[f"{name}_{k}"].tobytes(), (name, k)
    assert gr.DEFAULT.lo == gr.LO and gr.DEFAULT.ring_size == gr.RING_SIZE

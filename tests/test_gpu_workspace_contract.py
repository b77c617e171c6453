"""The C ABI's workspace contract: "the caller owns the scratch" (include/icpflow_hip.h).

Every other test of the suite reaches the library through `_lib.workspace()`: a grow-only cache of at least 1 MiB whose
cached size -- not the size asked for -- travels as `ws_bytes`, still holding what earlier calls left in it.  Here every
entry point runs the way a C caller runs it: on EXACTLY `*_workspace_bytes()` bytes, filled with a poison, between two
4 MiB guards in the same allocation (large against every region stride of a carve, small against the device), with its
outputs between guards as well.  Each case is run (a) the ordinary way -- the result the parity tests pin against the
oracle -- and (b) guarded under the poisons 0x00, 0xA5 and 0xFF (NaN floats, -1 integers), and asserts

  * status 0, every guard byte of workspace and outputs intact (a failure names the first / last changed offset relative
    to the end of the buffer, i.e. the region of the carve);
  * every output bit-identical to (a) (compared as bytes: `torch.equal` that also holds for NaN rows of empty pairs);
  * the same bits with the workspace base 16 bytes further (api.hip's check_ws refuses a base that is not 16-byte aligned
    and asks for no more; the clustering and frame entry points make no check at all);
  * `ws_bytes = need - 1` refused with ICPFLOW_E_WORKSPACE before anything is written (pre-filled outputs untouched).

The two anchor shapes (config 2; the first 16 pairs of the ragged 10^4-point batch) compare the guarded 0xFF run with the
oracle exactly as tests/test_gpu_fullsize.py does (its helpers, its thresholds), so that the module does not rest on
self-comparison alone.

The poisons are the outermost parameter (ids p00, pA5, pFF): on a shared GPU run them as three invocations, `-k p00`
first -- a poisoned word that a kernel polls on would be a hang, not a failed assert.

Who initialises what (read from the sources before the first poisoned run; "first touch" = the launch or memset of the
call that writes the region before anything of the call reads it):

  struct Workspace (csrc/api.hip)          first touch
  lenA, lenC, swap                         count_pair / the vote's sort (PairCountFuse) / sort_clouds selfCount
  bins                                     hipMemsetAsync in launch_hist_vote(_sorted) (hist.hip)
  volA, volB, peakVotes, peakIdx, cand     launch_hist_peaks_u32 (written, then read)
  partial                                  the scan / sweep that the following pick / select / epilogue reads
  scoreAccum, ticketScratch, shareCount    accumBytes: count_pair or the vote's sort (hist_icp*); estimate_init_pose clears
                                           scoreAccum in count_pair, leaves sweepTicket NULL and shareCountClean 0, so
                                           the sweeps memset shareCount themselves (nn.hip), as in apply_icp / match_eval
  Tinit, M                                 score_pick / the copy of d_init; launch_compose
  state                                    icp_kernel's first iteration (every pair, also the empty ones)
  ctrl (+ HelpPair[B], tag, owner)         icp_ctrl_bytes: count_pair / the vote's sort / launch_icp's memset
  helpState, helpOut                       published by the owner / helper before the tag that announces them
  grid.origin, start, cursor, pts          grid_build_kernel (search grid) / the sorts (sweep)
  grid.sortX, sortYsoa, sortXsoa, axis     sort_clouds_kernel / the chunked sorts, padding included
  zsortA, zsortC, voteKey, zckey, zcidx    zsort_kernel / launch_zsort_chunked
  voteWork, pairOrder                      vote_plan_kernel (pairOrder is handed on only when it ran: `planned`)
  grid.ckey, cidx, pairBox                 the chunked sorts; count_pair (pairBox handed on only when it wrote them)
  grid.scoreList                           the pruned scoring's deciding launch, counted by sweepTicket
  grid.occHdr, occBits                     launch_occupancy (occReady says so)
  grid.shareBest                           written by every sharing block before its count in shareCount
  pairTab                                  launch_sweep_pair_table (grid.pairTab set only when it ran)
  history                                  icp_kernel, row by row; readers stop at the iteration the tallies name
  team.wgPair, wgRank, teamSize, next,     icp_team_plan_kernel (all maxWG slots, all B pairs; arrived = 0): the only
  arrived                                  words a team member polls on; the helpers poll on `ctrl` words
  team.mom                                 team_publish before the arrival it is read behind
  icpSplit                                 icp_split_kernel (list, count, floor) before the second launch reads them

  table.hip   dict, start, rowOf, counts   table_dict_kernel / table_count_kernel / table_scan_kernel, in that order
  cluster.hip keyIn, valIn, firstRow, rootOf: dbscan_key_kernel; keyOut, valOut, sortTmp: rocprim; sorted: gather;
              runs, core: dbscan_core_kernel; parent: dbscan_hook_kernel (every row, before the first find);
              chunkRoot: flatten; rank: dbscan_rank_kernel
  hdbscan.hip keyIn, valIn: hdb_key_kernel; keyOut, valOut, sortTmp: rocprim; sorted, parent, comp, numComp, giant:
              hdb_gather_kernel; bmin .. preMaxX: the chunk kernels; core2: hdb_core_kernel; compW, compKey, chunkComp:
              hdb_round_init_kernel; bestW2, bestKey, bestQ: hdb_scan_kernel; compSize: hdb_select_kernel
  frame.hip   carves the three libraries' workspaces above out of the caller's scratch and fills its own tables first

Result: every region written before read: yes, with one exception that no kernel reads: icpflow_icp copies the WHOLE
history to options.d_icp_history, i.e. also float 15 of every record (written by nobody) and the rows of iterations that
were not reached -- both documented as unused / unspecified in the header, and the only caller-visible words that depend
on what the scratch held.  The t_history comparison below therefore covers the 15 named floats of the executed rows.
No fix to the carve or to a clear was needed.
"""
import contextlib
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

from icp_flow_amd import _lib, frame_pairs, synthetic, utils_check, utils_cluster, utils_hist, utils_icp, utils_match  # noqa: E402
from icp_flow_amd import utils_icp_pytorch3d as p3d  # noqa: E402
from icp_flow_amd.utils_icp import _icp_options  # noqa: E402
from oracle import reference_path as rp  # noqa: E402
from test_gpu_fullsize import C, DETERMINED_TOL, TOL_M, _all_host_threads, _smaller_first, displacement  # noqa: E402
from test_gpu_narrow_kernel import sort_codes  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 4 << 20          # bytes on either side: a condition (see above), not a measurement
GUARD_BYTE = 0x3C
OUT_FILL = 0x6B          # what an output holds before the call
E_WORKSPACE = -2         # ICPFLOW_E_WORKSPACE
POISONS = [pytest.param(0x00, id="p00"), pytest.param(0xA5, id="pA5"), pytest.param(0xFF, id="pFF")]
_live = []               # every guarded buffer not checked yet


def G(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---------------------------------------------------------------------------------------------------- the harness
class Guarded:
    """ONE device allocation [front guard | nbytes | back guard]: `.view` is the exact-size middle (base 256-aligned,
    + shift), filled with `poison`."""

    def __init__(self, nbytes, poison, shift=0, name="workspace", keep=False):
        self.nbytes, self.name, self.keep = int(nbytes), name, keep     # keep: checked by EVERY check_all() until the test ends
        self.raw = torch.empty(GUARD + 256 + shift + self.nbytes + GUARD, dtype=torch.uint8, device=DEV)
        self.raw.fill_(GUARD_BYTE)
        base = self.raw.data_ptr()
        self.start = (base + GUARD + 255) // 256 * 256 - base + shift
        self.view = self.raw[self.start:self.start + self.nbytes]
        self.view.fill_(poison)
        _live.append(self)

    def as_(self, dtype, *shape):
        return self.view.view(dtype).view(*shape)

    def check(self):
        torch.cuda.synchronize()
        end = self.start + self.nbytes
        for side, part, first in (("front", self.raw[:self.start], 0), ("back", self.raw[end:], end)):
            bad = torch.nonzero(part != GUARD_BYTE).flatten()
            assert bad.numel() == 0, (f"{self.name} ({self.nbytes} bytes): {bad.numel()} bytes of the {side} guard changed, offsets "
                                      f"{int(bad[0]) + first - end:+d} .. {int(bad[-1]) + first - end:+d} relative to the end of the buffer")

    def untouched(self, fill):
        torch.cuda.synchronize()
        return bool((self.view == fill).all())


def guarded(nbytes, poison, shift=0, name="workspace"):
    g = Guarded(nbytes, poison, shift, name)
    return g.view, g.check


def check_all():
    for g in list(_live):
        g.check()
    _live[:] = [g for g in _live if g.keep]


@pytest.fixture(autouse=True)
def every_guard_is_checked():
    _live.clear()
    yield
    check_all()
    _live.clear()


@contextlib.contextmanager
def exact_workspaces(poison, shift=0, short_batch=None):
    """Every Python-level path on the contract: `_lib.workspace` / `_lib.workspaces` hand out exact-size guarded views, so
    that `ws.numel() == need` reaches the library; the guards are checked when the block ends."""
    def workspace(device, nbytes):
        return Guarded(nbytes, poison, shift).view

    def workspaces(device, sizes):
        return [Guarded(n - (1 if k == short_batch else 0), poison, shift, f"workspace of batch {k}").view for k, n in enumerate(sizes)]

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "workspace", workspace)
        mp.setattr(_lib, "workspaces", workspaces)
        yield
    check_all()


def same(a, b):
    """Bit identity (the project asserts run-to-run bit identity for all of these: no tolerance)."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def out_buffer(dtype, *shape, keep=False):
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = Guarded(n, OUT_FILL, name=f"output {dtype} {list(shape)}", keep=keep)
    return g, g.as_(dtype, *shape)


def args_of(N, cap=50, tf=2.0, stop="reference"):
    a = rp.default_args(max_points=N, icp_max_iterations=cap, icp_stop_mode=stop)
    a.translation_frame = tf
    return a


def edges(a):
    ex, ey, ez = utils_hist.bin_edges(a, DEV)
    return (ex, ey, ez), (len(ex), len(ey), len(ez))


P = _lib.ptr


# ------------------------------------------------------------------------- the entry points, called as the wrappers call them
def c_hist_icp_eval(a, s, d, poison, shift=0, short=0):
    """-> (status, flat float32 [30 B + 1], its guard)"""
    B, N, _ = s.shape
    (ex, ey, ez), lens = edges(a)
    max_it, rel, stop = _icp_options(a)
    need = _lib.workspace_bytes(B, N, lens)
    ws = Guarded(need, poison, shift)
    og, flat = out_buffer(torch.float32, 30 * B + 1)
    at = [ctypes.c_void_p(flat.data_ptr() + 4 * B * c) for c in utils_match._EVAL_COLS]
    rc = _lib._L.icpflow_hist_icp_eval(P(s), P(d), B, N, P(ex), lens[0], P(ey), lens[1], P(ez), lens[2], float(a.thres_dist // 2),
                                       float(a.thres_dist), max_it, rel, stop, at[0], at[7], at[1], at[2], at[3], at[4], at[5], at[6],
                                       P(ws.view), need - short, _lib.stream(DEV), _lib.opt())
    return rc, flat, og


def c_hist_icp(a, s, d, poison, shift=0, short=0):
    B, N, _ = s.shape
    (ex, ey, ez), lens = edges(a)
    max_it, rel, stop = _icp_options(a)
    need = _lib.workspace_bytes(B, N, lens)
    ws = Guarded(need, poison, shift)
    (g1, T), (g2, it) = out_buffer(torch.float32, B, 4, 4), out_buffer(torch.int32, 1)
    rc = _lib._L.icpflow_hist_icp(P(s), P(d), B, N, P(ex), lens[0], P(ey), lens[1], P(ez), lens[2], float(a.thres_dist // 2),
                                  float(a.thres_dist), max_it, rel, stop, P(T), P(it), P(ws.view), need - short, _lib.stream(DEV), _lib.opt())
    return rc, (T, it), (g1, g2)


def c_init_pose(a, s, d, poison, shift=0, short=0):
    B, N, _ = s.shape
    (ex, ey, ez), lens = edges(a)
    need = _lib.workspace_bytes(B, N, lens)
    ws = Guarded(need, poison, shift)
    g, T = out_buffer(torch.float32, B, 4, 4)
    rc = _lib._L.icpflow_estimate_init_pose(P(s), P(d), B, N, P(ex), lens[0], P(ey), lens[1], P(ez), lens[2], float(a.thres_dist // 2),
                                            P(T), P(ws.view), need - short, _lib.stream(DEV), _lib.opt())
    return rc, (T,), (g,)


def c_apply_icp(a, s, d, init, poison, shift=0, short=0):
    B, N, _ = s.shape
    max_it, rel, stop = _icp_options(a)
    need = _lib.workspace_bytes(B, N)
    ws = Guarded(need, poison, shift)
    (g1, T), (g2, it) = out_buffer(torch.float32, B, 4, 4), out_buffer(torch.int32, 1)
    rc = _lib._L.icpflow_apply_icp(P(s), P(d), P(init), B, N, float(a.thres_dist), max_it, rel, stop, P(T), P(it), P(ws.view),
                                   need - short, _lib.stream(DEV), _lib.opt())
    return rc, (T, it), (g1, g2)


def c_match_eval(a, s, d, T, poison, shift=0, short=0):
    B, N, _ = s.shape
    need = _lib.workspace_bytes(B, N)
    ws = Guarded(need, poison, shift)
    outs = [out_buffer(torch.float32, B, 2) for _ in range(4)] + [out_buffer(torch.float32, B, 3) for _ in range(2)]
    o = [t for _, t in outs]
    rc = _lib._L.icpflow_match_eval(P(s), P(d), P(T), B, N, float(a.thres_dist), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4]), P(o[5]),
                                    P(ws.view), need - short, _lib.stream(DEV), _lib.opt())
    return rc, tuple(o), tuple(g for g, _ in outs)


def c_icp(s, d, thres, cap, poison, shift=0, short=0, history=False, scale=False):
    """icpflow_icp as iterative_closest_point calls it -> R, T, rmse, [iterations, converged](, t_history records)(, s)"""
    B, N, _ = s.shape
    need = _lib.workspace_bytes(B, N)
    ws = Guarded(need, poison, shift)
    bufs = [out_buffer(torch.float32, B, 3, 3), out_buffer(torch.float32, B, 3), out_buffer(torch.float32, B), out_buffer(torch.int32, 2)]
    if history:
        bufs.append(out_buffer(torch.float32, cap, B, 16))
    if scale:
        bufs.append(out_buffer(torch.float32, B))
    o = [t for _, t in bufs]
    with _lib.options(icp_history=o[4] if history else None, icp_scale=o[-1] if scale else None):
        rc = _lib._L.icpflow_icp(P(s), P(d), None, B, N, float(thres), int(cap), 1e-6, 0, P(o[0]), P(o[1]), P(o[2]), P(o[3][0:1]),
                                 P(o[3][1:2]), P(ws.view), need - short, _lib.stream(DEV), _lib.opt())
    return rc, tuple(o), tuple(g for g, _ in bufs)


def contract(call, want, poison, history_rows=None, served=None, also=()):
    """The four assertions of a case.  `call(poison, shift, short)` -> (status, outputs, their guards);
    `want`: the outputs of the ordinary run; served(): further assertions after every served call; also: guarded outputs
    the options of the call name, which a refused call must leave alone as well."""
    for shift in (0, 16):
        rc, got, _ = call(poison, shift, 0)
        assert rc == 0, (rc, _lib._L.icpflow_last_error())
        check_all()
        got = got if isinstance(got, tuple) else (got,)
        if history_rows is not None:      # (t_history: the rows of the executed iterations are defined, the others scratch)
            # (... and of a record the 15 floats the header names; the 16th is a copy of a workspace word no kernel writes)
            got = tuple(g[:history_rows, :, :15] if g.dim() == 3 and g.shape[-1] == 16 else g for g in got)
            want = tuple(w[:, :, :15] if w.dim() == 3 and w.shape[-1] == 16 else w for w in want)
        assert same(got, want if isinstance(want, tuple) else (want,)), f"poison 0x{poison:02x}, workspace base + {shift}"
        if served is not None:
            served()
    for g in also:
        g.view.fill_(OUT_FILL)
    rc, _, guards = call(poison, 0, 1)
    assert rc == E_WORKSPACE and b"workspace" in _lib._L.icpflow_last_error(), rc
    guards = guards if isinstance(guards, tuple) else (guards,)
    assert all(g.untouched(OUT_FILL) for g in tuple(guards) + tuple(also)), "a refused call wrote to an output"
    ws = [g for g in _live if g.name == "workspace"]
    assert ws and all(g.untouched(poison) for g in ws), "a refused call wrote to the workspace"
    check_all()


# ---------------------------------------------------------------------------------------------------- the shape panel
def _one_point():
    S, D, _ = synthetic.make_batch(1, 64, seed=4)
    S[0, 1:], D[0, 1:] = np.array([1e8, 1e8, 1e8, 0], np.float32), np.array([1e8, 1e8, 1e8, 0], np.float32)
    return S, D


def _empty_clouds():
    S, D, _ = synthetic.make_batch(8, 256, seed=6, ragged=True, n_min=30)
    pad = np.array([1e8, 1e8, 1e8, 0], np.float32)
    S[2] = pad                 # an empty moving cloud
    D[4] = pad                 # an empty fixed cloud
    S[6], D[6] = pad, pad      # an all-padding pair
    return S, D


def _shells():
    """The 1100-point box shells of tests/test_gpu_narrow_kernel.py (a face across the longest axis): most of them sort along a
    direction key, so the launch takes the general kernel -- asserted, so that the two cases below stay two cases."""
    n, B = 1100, 128
    S, D, _ = synthetic.make_batch(B, n, seed=11)
    for k in range(B):
        r = np.random.default_rng(700 + k)
        ext = np.array([r.uniform(2.5, 5.0), r.uniform(1.2, 2.2), r.uniform(1.0, 2.0)])
        pts = synthetic._shell_points(r, ext, n)
        if k % 2:
            pts = pts[:, [1, 0, 2]]
        c = np.array([r.uniform(-30, 30), r.uniform(-30, 30), 0.8])
        t = np.array([r.uniform(-1, 1), r.uniform(-1, 1), 0.0])
        S[k, :, :3], S[k, :, 3] = (pts + c).astype(np.float32), 1.0
        D[k, :, :3], D[k, :, 3] = (pts + c + t + r.normal(0, 0.01, pts.shape)).astype(np.float32), 1.0
    assert (sort_codes(D) >= 3).mean() >= 0.5
    return S, D


def _masked():
    S, D, _ = synthetic.make_batch(300, 1100, seed=37)
    return S, D


MB = synthetic.make_batch
# name -> (clouds, keyword arguments of args_of, options of the call, extra device buffers the options name)
PANEL = {
    "allpairs_7x40": (lambda: MB(7, 40, seed=1)[:2], {}, {}),
    "config2_256x1024_vote_bins": (lambda: MB(256, 1024, seed=0)[:2], {}, {"vote_bins": True}),
    "general_kernel_128x1100": (_shells, {}, {}),
    "general_kernel_128x1100_no_dir_keys": (_shells, {}, {"no_dir_keys": True}),
    "share_scratch_600x2048": (lambda: MB(600, 2048, seed=31)[:2], {}, {}),
    "helpers_ragged_900x2048": (lambda: MB(900, 2048, seed=23, ragged=True, n_min=100)[:2], {}, {}),
    "helpers_ragged_900x2048_two_launch": (lambda: MB(900, 2048, seed=23, ragged=True, n_min=100)[:2], {}, {"two_launch": True}),
    "helpers_ragged_900x2048_no_persistent": (lambda: MB(900, 2048, seed=23, ragged=True, n_min=100)[:2], {}, {"no_persistent": True}),
    "helpers_ragged_900x2048_no_helpers": (lambda: MB(900, 2048, seed=23, ragged=True, n_min=100)[:2], {}, {"no_helpers": True}),
    "config4_shard_1024x2048": (lambda: MB(1024, 2048, seed=0)[:2], {}, {}),
    "config4_shard_1024x2048_two_launch": (lambda: MB(1024, 2048, seed=0)[:2], {}, {"two_launch": True}),
    "team_mom_255x1024": (lambda: tuple(x[:255] for x in MB(257, 1024, seed=3)[:2]), {}, {}),
    "team_mom_257x1024": (lambda: MB(257, 1024, seed=3)[:2], {}, {}),
    "teams_ragged_12x4000": (lambda: MB(12, 4000, seed=7, ragged=True, n_min=500)[:2], {}, {}),
    "teams_ragged_12x4000_no_teams": (lambda: MB(12, 4000, seed=7, ragged=True, n_min=500)[:2], {}, {"no_teams": True}),
    "teams_matched_48x10000": (lambda: MB(48, 10000, seed=5, ragged="matched", n_min=200)[:2], {"cap": 100}, {}),
    "teams_independent_16x10000": (lambda: MB(16, 10000, seed=0, ragged=True, n_min=20)[:2], {"cap": 100}, {}),
    "teams_independent_16x10000_no_shared_scans": (lambda: MB(16, 10000, seed=0, ragged=True, n_min=20)[:2], {"cap": 100}, {"no_shared_scans": True}),
    "beyond_the_sort_2x16500": (lambda: MB(2, 16500, seed=2)[:2], {"cap": 20}, {}),
    "one_point_1x64": (_one_point, {}, {}),
    "empty_clouds_8x256": (_empty_clouds, {}, {}),
    "histogram_269_bins_24x700": (lambda: MB(24, 700, seed=13, ragged=True, n_min=40)[:2], {"tf": 13.36}, {}),
    "search_scan_40x300": (lambda: MB(40, 300, seed=17, ragged=True, n_min=30)[:2], {}, {"search": "scan"}),
    "search_grid_40x300": (lambda: MB(40, 300, seed=17, ragged=True, n_min=30)[:2], {}, {"search": "grid"}),
    "search_sweep_40x300": (lambda: MB(40, 300, seed=17, ragged=True, n_min=30)[:2], {}, {"search": "sweep"}),
    "fp32_reference_64x512": (lambda: MB(64, 512, seed=19)[:2], {}, {"arith": "fp32_reference"}),
    "per_pair_cap_200_20x1500": (lambda: MB(20, 1500, seed=29, ragged=True, n_min=200)[:2], {"cap": 200, "stop": "per_pair"}, {}),
    "pair_active_300x1100": (_masked, {}, {"pair_active": True}),
}
_clouds = {}


def clouds_of(case):
    make = PANEL[case][0]
    key = re.match(r".*?\d+x\d+", case).group(0)      # (the option variants of a shape share its clouds)
    if key not in _clouds:
        _clouds.clear()          # (one batch resident at a time: the long ones are hundreds of MiB)
        S, D = make()
        _clouds[key] = (G(S), G(D), S, D)
    return _clouds[key]


@pytest.mark.parametrize("case", list(PANEL))
@pytest.mark.parametrize("poison", POISONS)
def test_hist_icp_eval_on_an_exact_poisoned_workspace(poison, case):
    """icpflow_hist_icp_eval -- hist_icp_core and match_eval_core on one carve, the flat [30 B + 1] result -- over the panel."""
    _, kw, opts = PANEL[case]
    s, d, _, _ = clouds_of(case)
    B, N, _ = s.shape
    a = args_of(N, **kw)
    opts = dict(opts)
    lens = edges(a)[1]
    bins_want = bins_g = bins = None
    if opts.pop("vote_bins", False):
        bins_want = torch.zeros((B, lens[0] * lens[1] * lens[2]), dtype=torch.int32, device=DEV)
        bins_g, bins = out_buffer(torch.int32, B, lens[0] * lens[1] * lens[2], keep=True)
    if opts.pop("pair_active", False):
        opts["pair_active"] = G((np.arange(B) % 3 != 1).astype(np.uint8))
    with _lib.options(vote_bins=bins_want, **opts):
        want, _ = utils_match._hist_icp_eval_flat(a, s, d)
    torch.cuda.synchronize()
    with _lib.options(vote_bins=bins, **opts):
        contract(lambda p, sh, short: c_hist_icp_eval(a, s, d, p, sh, short), want, poison,
                 served=(lambda: None) if bins is None else (lambda: _assert_same(bins, bins_want)), also=() if bins is None else (bins_g,))


def _assert_same(a, b):
    assert same(a, b)


ENTRY_SHAPES = {"config2_256x1024": lambda: MB(256, 1024, seed=0)[:2],
                "ragged_40x3000": lambda: MB(40, 3000, seed=47, ragged=True, n_min=300)[:2],
                "small_9x50": lambda: MB(9, 50, seed=8, ragged=True, n_min=10)[:2]}


@pytest.mark.parametrize("shape", list(ENTRY_SHAPES))
@pytest.mark.parametrize("poison", POISONS)
def test_every_other_entry_point_with_guarded_outputs(poison, shape):
    """icpflow_hist_icp, _estimate_init_pose, _apply_icp, _match_eval (scans and sweeps) and _icp with t_history and a scale,
    each against its wrapper's ordinary result, outputs between guards."""
    S, D = ENTRY_SHAPES[shape]()
    s, d = G(S), G(D)
    N = s.shape[1]
    a = args_of(N)
    T, it = utils_match.hist_icp(a, s, d, return_iterations=True)
    contract(lambda p, sh, short: c_hist_icp(a, s, d, p, sh, short), (T, it), poison)
    init = utils_hist.estimate_init_pose(a, s, d)
    contract(lambda p, sh, short: c_init_pose(a, s, d, p, sh, short), (init,), poison)
    with _lib.options(no_sorted_vote=True, no_score_prune=True):
        init2 = utils_hist.estimate_init_pose(a, s, d)
        contract(lambda p, sh, short: c_init_pose(a, s, d, p, sh, short), (init2,), poison)
    Ta, ita = utils_icp.apply_icp(a, s, d, init, return_iterations=True)
    contract(lambda p, sh, short: c_apply_icp(a, s, d, init, p, sh, short), (Ta, ita), poison)
    ev = utils_match.match_eval(a, s, d, T)
    contract(lambda p, sh, short: c_match_eval(a, s, d, T, p, sh, short), tuple(ev), poison)
    with _lib.options(no_eval_sweep=True):
        ev2 = utils_match.match_eval(a, s, d, T)
        contract(lambda p, sh, short: c_match_eval(a, s, d, T, p, sh, short), tuple(ev2), poison)
    for scale in (False, True):
        sol = p3d.iterative_closest_point(s, d, thres=a.thres_dist, max_iterations=50, estimate_scale=scale)
        n = sol.converged.iterations
        want = (sol.RTs.R, sol.RTs.T, sol.rmse, sol.converged._flags, sol.t_history.records()) + ((sol.RTs.s,) if scale else ())
        contract(lambda p, sh, short: c_icp(s, d, a.thres_dist, 50, p, sh, short, history=True, scale=scale), want, poison, history_rows=n)


@pytest.mark.parametrize("poison", POISONS)
def test_python_level_paths_on_exact_workspaces(poison):
    """The wrappers themselves with `_lib.workspace` handing out exact-size guarded views: hist_icp, hist_icp_eval,
    estimate_init_pose, topk_nms, iterative_closest_point, apply_icp, match_eval, per-pair stop, one launch per iteration."""
    S, D, _ = MB(90, 2048, seed=23, ragged=True, n_min=100)
    s, d = G(S), G(D)
    a, ap = args_of(2048), args_of(2048, stop="per_pair")

    def everything():
        T, it = utils_match.hist_icp(a, s, d, return_iterations=True)
        Te, ev, ite = utils_match.hist_icp_eval(a, s, d, return_iterations=True)
        init = utils_hist.estimate_init_pose(a, s, d)
        votes = utils_hist.topk_nms(torch.arange(2 * 9 * 9 * 3, dtype=torch.float32, device=DEV).reshape(2, 9, 9, 3) % 7)
        sol = p3d.iterative_closest_point(s, d, thres=a.thres_dist, max_iterations=30)
        Ta = utils_icp.apply_icp(a, s, d, init)
        m = utils_match.match_eval(a, s, d, T)
        Tp = utils_match.hist_icp(ap, s, d)
        with _lib.options(no_speculative=True):
            Tn = utils_match.hist_icp(a, s, d)
        return (T, it, Te, *ev, ite, init, *votes, sol.RTs.R, sol.RTs.T, sol.rmse, sol.converged._flags, Ta, *m, Tp, Tn)

    want = everything()
    for shift in (0, 16):
        with exact_workspaces(poison, shift):
            got = everything()
        assert same(got, want), f"workspace base + {shift}"


@pytest.mark.parametrize("poison", POISONS)
def test_hist_icp_many_every_workspace_guarded(poison):
    """Six batches of different B in flight (the shapes of test_hist_icp_many_equals_separate_calls), each on its own exact
    guarded workspace; the guards are checked after the join."""
    N = 1024
    a = args_of(N)
    shapes = [(256, False, 0), (64, True, 300), (256, False, 256), (300, True, 600), (17, False, 900), (256, False, 512)]
    batches = [MB(B, N, seed=0, first=first, ragged=r, n_min=40) for B, r, first in shapes]
    srcs, dsts = [G(b[0]) for b in batches], [G(b[1]) for b in batches]
    want = [utils_match.hist_icp(a, s_, d_, return_iterations=True) for s_, d_ in zip(srcs, dsts)]
    for shift in (0, 16):
        with exact_workspaces(poison, shift):
            outs, iters = utils_match.hist_icp_many(a, srcs, dsts, return_iterations=True)
            assert len(_live) == 6
        for (T0, it0), T1, it1 in zip(want, outs, iters):
            assert same((T0, it0), (T1, it1)), f"workspace base + {shift}"
    # one byte short on batch 3: the call is refused there (the batches in front of it are in flight and joined), nothing
    # beyond any workspace is touched and the short workspace itself is not written
    with exact_workspaces(poison, short_batch=3):
        with pytest.raises(RuntimeError, match=r"code -2"):
            utils_match.hist_icp_many(a, srcs, dsts)
        torch.cuda.synchronize()
        assert [g for g in _live if g.name == "workspace of batch 3"][0].untouched(poison)


# ---------------------------------------------------------------------------------------------------- the clustering carves
def _frame():
    d = synthetic.make_frame_pair(seed=12, n_objects=6, n_max=300, n_background=600)
    return d


def _table_pair(ps, ls, pd, ld, poison, short=0, shift=0):
    R = utils_check.TABLE_ROWS
    MA, MB_ = len(ls), len(ld)
    need = int(_lib._L.icpflow_cluster_table_pair_workspace_bytes(MA, MB_, R))
    ws = Guarded(need, poison, shift)
    bufs = [out_buffer(torch.int64, MA), out_buffer(torch.float64, 1 + R * 9), out_buffer(torch.int64, MB_), out_buffer(torch.float64, 1 + R * 9)]
    o = [t for _, t in bufs]
    rc = _lib._L.icpflow_cluster_table_pair(P(ps), P(ls), MA, P(o[0]), o[1].data_ptr() + 8, P(o[1]), P(pd), P(ld), MB_, P(o[2]),
                                            o[3].data_ptr() + 8, P(o[3]), R, P(ws.view), need - short, _lib.stream(DEV))
    return rc, o, [g for g, _ in bufs]


def _table(ps, ls, poison, short=0, shift=0):
    R = utils_check.TABLE_ROWS
    M = len(ls)
    need = int(_lib._L.icpflow_cluster_table_workspace_bytes(M, R))
    ws = Guarded(need, poison, shift)
    bufs = [out_buffer(torch.int64, M), out_buffer(torch.float64, 1 + R * 9)]
    o = [t for _, t in bufs]
    rc = _lib._L.icpflow_cluster_table(P(ps), P(ls), M, P(o[0]), o[1].data_ptr() + 8, R, P(o[1]), P(ws.view), need - short, _lib.stream(DEV))
    return rc, o, [g for g, _ in bufs]


def _table_rows(packed):
    """What a table call defines of its packed buffer: the int32 count and that many rows."""
    L = int(packed[0:1].view(torch.int32)[0])
    return (packed[0:1].view(torch.int32)[0:1].clone(), packed[1:1 + max(L, 0) * 9])


@pytest.mark.parametrize("poison", POISONS)
def test_cluster_tables_on_exact_poisoned_workspaces(poison):
    """icpflow_cluster_table / _pair: the demo frame's labels, a 1-point and a 2-point cloud, more labels than TABLE_ROWS."""
    f = _frame()
    clouds = [(G(f["points_src"][:, :3].astype(np.float32)), G(f["labels_src"].astype(np.float32))),
              (G(f["points_dst"][:, :3].astype(np.float32)), G(f["labels_dst"].astype(np.float32))),
              (G(np.array([[1, 2, 3]], np.float32)), G(np.array([4], np.float32))),
              (G(np.array([[1, 2, 3], [2, 2, 2]], np.float32)), G(np.array([7, -1], np.float32))),
              (G(np.random.default_rng(0).normal(size=(3000, 3)).astype(np.float32)), G((np.arange(3000) % 700).astype(np.float32)))]
    for ps, ls in clouds:
        t = utils_check.ClusterTable(ps, ls, fetch=False)
        torch.cuda.synchronize()
        for shift in (0, 16):
            rc, o, guards = _table(ps, ls, poison, shift=shift)
            assert rc == 0
            check_all()
            assert same(_table_rows(o[1]), _table_rows(t._packed)), shift
            if int(_table_rows(o[1])[0]) >= 0:      # (more labels than TABLE_ROWS: the count says so, the order is not defined)
                assert same(o[0], t.order), shift
        rc, o, guards = _table(ps, ls, poison, short=1)
        assert rc == E_WORKSPACE and all(g.untouched(OUT_FILL) for g in guards)
        check_all()
    for (pa, la), (pb, lb) in ((clouds[0], clouds[1]), (clouds[2], clouds[3]), (clouds[4], clouds[0])):
        st, dt = utils_check.ClusterTable.pair(pa, la, pb, lb, fetch=False)
        torch.cuda.synchronize()
        for shift in (0, 16):
            rc, o, guards = _table_pair(pa, la, pb, lb, poison, shift=shift)
            assert rc == 0
            check_all()
            assert same(_table_rows(o[1]), _table_rows(st._packed)) and same(_table_rows(o[3]), _table_rows(dt._packed)), shift
            assert int(_table_rows(o[1])[0]) < 0 or same(o[0], st.order), shift
            assert int(_table_rows(o[3])[0]) < 0 or same(o[2], dt.order), shift
        rc, o, guards = _table_pair(pa, la, pb, lb, poison, short=1)
        assert rc == E_WORKSPACE and all(g.untouched(OUT_FILL) for g in guards)
        check_all()
    for shift in (0, 16):                 # ... and the wrappers, host tables included
        with exact_workspaces(poison, shift):
            st, dt = utils_check.ClusterTable.pair(*clouds[0], *clouds[1])
            one = utils_check.ClusterTable(*clouds[0])
        assert np.array_equal(st.h_count, one.h_count) and np.array_equal(st.h_mean, one.h_mean)


def _dbscan(pts, mask, eps, minpts, poison, short=0, shift=0):
    n = len(pts)
    need = int(_lib._L.icpflow_dbscan_workspace_bytes(n))
    ws = Guarded(need, poison, shift)
    bufs = [out_buffer(torch.int32, n), out_buffer(torch.int32, n), out_buffer(torch.int32, 1)]
    o = [t for _, t in bufs]
    rc = _lib._L.icpflow_dbscan(P(pts), pts.shape[1], P(mask), n, float(eps), int(minpts), P(o[0]), P(o[1]), P(o[2]), P(ws.view),
                                need - short, _lib.stream(DEV))
    return rc, o, [g for g, _ in bufs]


def _mst(pts, mask, k, poison, short=0, shift=0):
    n = len(pts)
    need = int(_lib._L.icpflow_hdbscan_mst_workspace_bytes(n))
    ws = Guarded(need, poison, shift)
    bufs = [out_buffer(torch.float64, n), out_buffer(torch.int32, n), out_buffer(torch.int32, n), out_buffer(torch.float64, n),
            out_buffer(torch.int32, 2)]
    o = [t for _, t in bufs]
    rc = _lib._L.icpflow_hdbscan_mst(P(pts), pts.shape[1], P(mask), n, int(k), 0.25, P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(o[4][0:1]),
                                     P(o[4][1:2]), P(ws.view), need - short, _lib.stream(DEV))
    return rc, o, [g for g, _ in bufs]


@pytest.mark.parametrize("poison", POISONS)
def test_dbscan_and_the_hdbscan_tree_on_exact_poisoned_workspaces(poison):
    """icpflow_dbscan / icpflow_hdbscan_mst: the demo frame's non-ground points (with and without a mask), a 1-point and a
    2-point cloud.  Labels, sizes, tree edges (as the set the wrapper returns: n_live - 1 of them) and core distances."""
    f = _frame()
    pts = G(f["points_src"][:, :3].astype(np.float32))
    mask = G((np.arange(len(pts)) % 5 != 0).astype(np.uint8))
    clouds = [(pts, None), (pts, mask), (G(np.array([[0, 0, 0]], np.float32)), None), (G(np.array([[0, 0, 0], [0.1, 0, 0]], np.float32)), None)]
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g10, g11 = np.load(os.path.join(golden, "g10_dbscan.npz")), np.load(os.path.join(golden, "g11_hdbscan.npz"))
    clouds += [(G(g10["small_2_points"]), G(g10["small_2_nonground"].astype(np.uint8))), (G(g11["crop_1_points"]), None)]
    for p, m in clouds:
        labels, sizes = utils_cluster.dbscan(p, 0.8, 2, m)
        for shift in (0, 16):
            rc, o, guards = _dbscan(p, m, 0.8, 2, poison, shift=shift)
            assert rc == 0
            check_all()
            nc = int(o[2][0])
            assert same(o[0], labels) and nc == len(sizes) and same(o[1][:nc], sizes), shift
        rc, o, guards = _dbscan(p, m, 0.8, 2, poison, short=1)
        assert rc == E_WORKSPACE and all(g.untouched(OUT_FILL) for g in guards)
        check_all()
        k = 1 if len(p) < 8 else 4
        want = utils_cluster.hdbscan_mst(p, k, m)
        # (the order in which the rounds append their edges is a race between blocks: the tree is the SET of its edges)
        key = lambda a_, b_, w_: sorted(zip(a_.tolist(), b_.tolist(), w_.tolist()))  # noqa: E731
        for shift in (0, 16):
            rc, o, guards = _mst(p, m, k, poison, shift=shift)
            assert rc == 0
            check_all()
            ne, nl = int(o[4][0]), int(o[4][1])
            assert nl == want["n_live"] and ne == len(want["a"]), shift
            assert same(o[0], want["core2"]), shift
            assert key(o[1][:ne], o[2][:ne], o[3][:ne]) == key(want["a"], want["b"], want["w2"]), shift
        rc, o, guards = _mst(p, m, k, poison, short=1)
        assert rc == E_WORKSPACE and all(g.untouched(OUT_FILL) for g in guards)
        check_all()
    l1, s1 = utils_cluster.dbscan(pts, 0.8, 2, mask)
    for shift in (0, 16):
        with exact_workspaces(poison, shift):
            l2, s2 = utils_cluster.dbscan(pts, 0.8, 2, mask)
            t2 = utils_cluster.hdbscan_mst(pts, 4, mask)
        assert same((l1, s1), (l2, s2)) and t2["n_live"] == int(mask.sum())


# ---------------------------------------------------------------------------------------------------- frame pairs
def _frame_pair():
    d = _frame()
    fp = frame_pairs.FramePair(d["points_src"], d["points_dst"], d["labels_src"], d["labels_dst"], d["pose"], d["gt_flow"])
    return fp, frame_pairs.default_args(max_points=256)


@pytest.mark.parametrize("poison", POISONS)
def test_association_stages_on_exact_workspaces(poison):
    """The Python host of a frame pair (icpflow_register_stage / icpflow_associate_frame, the device-side association) with
    every workspace exact and poisoned: matched pairs, transforms and flow of the ordinary run."""
    fp, a = _frame_pair()
    a = SimpleNamespace(**vars(a))
    a.native_host = False
    torch.manual_seed(0)
    want = frame_pairs.register_frame_pair(a, fp, DEV)
    torch.cuda.synchronize()
    for shift in (0, 16):
        torch.manual_seed(0)
        called, plain = [], _lib.call
        with exact_workspaces(poison, shift), pytest.MonkeyPatch.context() as mp:
            mp.setattr(_lib, "call", lambda name, *args: (called.append(name), plain(name, *args))[1])
            got = frame_pairs.register_frame_pair(a, fp, DEV)
            torch.cuda.synchronize()
            assert len(_live) >= 2
        # (the Python host registers stage 1 and hands stage 2 to the association call; the begin -> finish hand-over of a
        # stage belongs to icpflow_track_frame alone: the next test)
        assert "icpflow_register_stage" in called and "icpflow_associate_frame" in called and "icpflow_cluster_table_pair" in called, called
        for k in ("pairs", "transformations", "flow"):
            assert same(torch.as_tensor(got[k]), torch.as_tensor(want[k])), (k, shift)


@pytest.mark.parametrize("poison", POISONS)
def test_track_frame_from_a_too_small_scratch_upward(poison):
    """icpflow_track_frame through its refusal protocol: from a scratch far too small, each refusal names what the frame
    pair needs (`*scratch_needed`), and the next call gets exactly that many poisoned bytes between guards.  A refusal --
    at whichever of its three depths, the later ones behind launches already enqueued -- leaves rows, transforms and flow
    as they were; the served call gives the ordinary call's bits, also with the scratch base at +16 and without the
    overlap of the stages (the begin -> finish hand-over of stage 2's workspace against one call per stage); one byte less
    than what served is refused again."""
    fp, a = _frame_pair()
    want = frame_pairs.register_frame_pair_native(a, fp, DEV)
    assert frame_pairs._served(want)
    torch.cuda.synchronize()
    a = SimpleNamespace(**vars(a))
    a.translation_frame = frame_pairs.frame_translation(a, fp.pose_exact, fp.gap)
    ps, pd = G(fp.points_src[:, :3].astype(np.float32)), G(fp.points_dst[:, :3].astype(np.float32))
    ls, ld = G(fp.labels_src).float().contiguous(), G(fp.labels_dst).float().contiguous()
    pose = G(fp.pose).float().contiguous()
    reg, keep = utils_match._registration(a, DEV)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    par = _lib.FrameParams(ctypes.sizeof(_lib.FrameParams), 0, None, int(a.max_points), int(a.min_cluster_size), f32(a.translation_frame),
                           f32(a.thres_box), f32(a.thres_iou), f32(a.thres_rot * 90.0), f32(a.thres_error), 1, 1024)

    def call(size, shift):
        """-> status, bytes asked for, pairs, (rows, T, flow), their guards"""
        outs = [out_buffer(torch.float32, 1024, 10, keep=True), out_buffer(torch.float32, 1024, 4, 4, keep=True),
                out_buffer(torch.float32, len(ps), 3, keep=True)]
        (_, rows), (_, T), (_, flow) = outs
        pairs, need = ctypes.c_int32(0), ctypes.c_size_t(0)
        scratch = Guarded(size, poison, shift, name="frame scratch")
        rc = _lib._L.icpflow_track_frame(P(ps), P(ls), len(ps), P(pd), P(ld), len(pd), ctypes.byref(reg), ctypes.byref(par), P(rows), P(T),
                                         ctypes.byref(pairs), P(ps), P(pose), P(flow), P(scratch.view), size, ctypes.byref(need),
                                         _lib.stream(DEV), _lib.opt())
        check_all()
        return rc, int(need.value), int(pairs.value), (rows, T, flow), [g for g, _ in outs]

    def served(got, n):
        assert n == len(want["pairs"])
        assert same(got[0][:n], want["pairs"]) and same(got[1][:n], want["transformations"]) and same(got[2], want["flow"])

    for overlap in (True, False):
        with _lib.options(teams_half_gpu=True, no_shared_scans=True, no_stage_overlap=not overlap):
            size, refusals, rc = 4096, [], E_WORKSPACE
            for _ in range(6):
                rc, need, n, got, guards = call(size, 0)
                if rc != E_WORKSPACE:
                    break
                assert need > size, (need, size)
                assert all(g.untouched(OUT_FILL) for g in guards), f"refused with {size} bytes, but an output was written"
                refusals.append(size)
                size = need
            print(f"icpflow_track_frame (stage overlap {overlap}): refused at {refusals}, served with {size} bytes")
            assert rc == 0 and refusals, (rc, _lib._L.icpflow_last_error())
            served(got, n)
            rc, need, n, got, guards = call(size, 16)
            assert rc == 0, (rc, _lib._L.icpflow_last_error())
            served(got, n)
            rc, need, n, got, guards = call(size - 1, 0)
            assert rc == E_WORKSPACE and need == size, (rc, need, size)
            assert all(g.untouched(OUT_FILL) for g in guards), "refused one byte short, but an output was written"
        _live.clear()


# ---------------------------------------------------------------------------------------------------- the anchors
def test_config2_guarded_run_vs_oracle():
    """Config 2 (256 x 1024) on an exact workspace poisoned with 0xFF against the oracle, as test_config2_full_batch_vs_oracle
    and test_config2_full_batch_initial_poses_equal_the_oracle do: initial poses equal, the iteration count of the
    fp64-Kabsch evaluation, every pair within 1e-5 m of it."""
    S, D, _ = MB(256, 1024, seed=0)
    a = rp.default_args(max_points=1024, icp_max_iterations=50)
    _all_host_threads()
    _, aux32 = rp.hist_icp(a, C(S), C(D), max_iterations=50, return_aux=True)
    T64, aux64 = rp.hist_icp(a, C(S), C(D), max_iterations=50, return_aux=True, kabsch_dtype=torch.float64, init=aux32["init"])
    s, d = G(S), G(D)
    rc, (init,), _ = c_init_pose(a, s, d, 0xFF)
    assert rc == 0
    rc, (T, it), _ = c_hist_icp(a, s, d, 0xFF)
    assert rc == 0
    check_all()
    assert np.array_equal(init.cpu().numpy(), aux32["init"].numpy())
    err64 = displacement(T.cpu().numpy(), T64.numpy(), S)
    print(f"iterations {int(it)} (fp64-Kabsch oracle {aux64['iterations']}), max displacement {err64.max():.2e} m")
    assert int(it) == aux64["iterations"]
    assert err64.max() < 1e-5


def test_ragged_16_pairs_guarded_run_vs_oracle():
    """The first 16 pairs of the ragged 10^4-point batch on an exact workspace poisoned with 0xFF, as
    test_ragged_real_shape_16_pairs_vs_oracle does."""
    S, D, _ = MB(16, 10000, seed=0, ragged=True, n_min=20)
    a = rp.default_args(max_points=10000, icp_max_iterations=100)
    _all_host_threads()
    T32, aux32 = rp.hist_icp(a, C(S), C(D), max_iterations=100, return_aux=True)
    T64, aux64 = rp.hist_icp(a, C(S), C(D), max_iterations=100, return_aux=True, kabsch_dtype=torch.float64, init=aux32["init"])
    rc, (T, it), _ = c_hist_icp(a, G(S), G(D), 0xFF)
    assert rc == 0
    rc, (init,), _ = c_init_pose(a, *[G(x) for x in _smaller_first(S, D)], 0xFF)
    assert rc == 0
    check_all()
    assert np.array_equal(init.cpu().numpy(), aux32["init"].numpy())
    T = T.cpu().numpy()
    err32, err64 = displacement(T, T32.numpy(), S), displacement(T, T64.numpy(), S)
    agree = displacement(T32.numpy(), T64.numpy(), S) < DETERMINED_TOL
    print(f"iterations {int(it)} (fp64-Kabsch oracle {aux64['iterations']}), vs fp64-Kabsch oracle {err64.max():.2e} m")
    assert int(it) == aux64["iterations"]
    assert err64.max() < 1e-5
    assert err32[agree].max() < TOL_M

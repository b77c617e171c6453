"""icpflow_ground_segment against the fp64 restatement of the method (tests/ground_restatement.py) on the scenes of
tests/ground_scenes.py: labels equal on every row that is not in an undetermined patch, decision codes, counts and revert
outcomes equal and mean, normal, d and singular values within 1e-9 on every determined patch -- two orders over the ~1e-11
that fp64 sums over at most 2 * 10^4 points and an eigen gap of at least 1e-3 allow.  Every figure is printed before it is
asserted."""
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

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def scene(name):
    pts, parts = gs.ALL[name]()
    return pts, parts, gr.segment(pts)


def run(pts):
    """-> (non-ground bool [n], table [504, 16]) as numpy, through the Python entry point with a resident tensor"""
    from icp_flow_amd import utils_ground
    labels, table = utils_ground.segment_ground_pypatchworkpp(torch.from_numpy(np.ascontiguousarray(pts)).to(DEV), return_table=True)
    assert labels.is_cuda and labels.dtype == torch.bool and table.is_cuda
    return labels.cpu().numpy(), table.cpu().numpy()


def compare(name, res, labels, table):
    keep, det = gr.rows_to_compare(res), gr.determined(res)
    want = res["table"]
    diff = np.abs(table[det][:, 2:12] - want[det][:, 2:12])
    diff = diff[~(np.isnan(table[det][:, 2:12]) & np.isnan(want[det][:, 2:12]))]
    print(f"{name}: rows {len(labels)}, compared {int(keep.sum())}, determined patches {int(det.sum())}, label mismatches "
          f"{int((labels[keep] != res['nonground'][keep]).sum())}, max |plane - restatement| {diff.max() if diff.size else 0.0:.3e}")
    assert (table[:, 0] == want[:, 0]).all()                                # the binning, row for row
    assert (labels[keep] == res["nonground"][keep]).all()
    for col in (1, 12, 13, 14):
        assert (table[det, col] == want[det, col]).all(), col
    assert (np.isnan(table[det][:, 2:12]) == np.isnan(want[det][:, 2:12])).all()
    assert not diff.size or diff.max() <= TOL
    small = want[:, 0] < gr.NUM_MIN_PTS
    assert (table[small, 1:] == 0).all()


def test_edges_of_the_binning():
    from icp_flow_amd import utils_ground
    pts, parts, res = scene("edges")
    labels, table = run(pts)
    compare("edges", res, labels, table)
    assert (labels == res["nonground"]).all() and labels[parts["special"]].all() and labels[parts["nine"]].all() and not labels[parts["ten"]].any()
    for n in (0, 1):
        out, tab = utils_ground.segment_ground_pypatchworkpp(torch.from_numpy(pts[40:40 + n]).to(DEV), return_table=True)
        assert out.shape == (n,) and out.all() and (tab.cpu().numpy()[:, 1:] == 0).all()
    far = np.float32([[70.0, 1.0, -1.7], [0.3, 0.2, -1.7], [np.nan, 0.0, 0.0]] * 30)
    out, tab = run(far)
    assert out.all() and (tab == 0).all()


@pytest.mark.parametrize("name", sorted(gs.SMALL))
def test_patch_chain_and_revert(name):
    pts, parts, res = scene(name)
    labels, table = run(pts)
    compare(name, res, labels, table)
    if name == "platform":                                                  # every outcome of the revert is present
        assert {(int(c), int(t)) for c, t in table[table[:, 12] == gr.CANDIDATE][:, 12:14]} == {(5, 1), (5, 2)}
        assert (labels == res["nonground"]).all()
    if name == "walls":
        assert table[gr.patch_index(0, 0, 2), 14] >= 400 and table[gr.patch_index(1, 1, 9), 14] == 0
        assert np.isnan(table[gr.patch_index(1, 2, 4), 5:12]).all() and table[gr.patch_index(0, 1, 5), 1] == 0


@pytest.mark.parametrize("name", sorted(gs.LARGE) + ["tied"])
def test_large_and_tied_and_permuted(name):
    pts, parts, res = scene(name)
    labels, table = run(pts)
    compare(name, res, labels, table)
    perm = np.random.default_rng(11).permutation(len(pts))
    again, _ = run(pts[perm])
    keep = gr.rows_to_compare(res)[perm]
    assert (again[keep] == labels[perm][keep]).all()


def test_reruns_and_streams_are_bit_identical():
    from icp_flow_amd import utils_ground
    pts, _, _ = scene("platform")
    x = torch.from_numpy(pts).to(DEV)
    first = utils_ground.segment_ground_pypatchworkpp(x, return_table=True)
    again = utils_ground.segment_ground_pypatchworkpp(x, return_table=True)
    torch.cuda.synchronize()
    streams, outs = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)], []
    for s in streams:
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            outs.append(utils_ground.segment_ground_pypatchworkpp(x, return_table=True))
    torch.cuda.synchronize()
    for got in [again] + outs:
        assert torch.equal(got[0], first[0]) and torch.equal(got[1].view(torch.int64), first[1].view(torch.int64))


def test_entry_forms_agree():
    from icp_flow_amd import utils_ground
    pts, _, res = scene("flat_boxes")
    a = SimpleNamespace(range_z=-1.75, ground_slack=0.3)
    want, _ = run(pts)
    from_f64 = utils_ground.segment_ground_pypatchworkpp(pts.astype(np.float64))
    assert isinstance(from_f64, np.ndarray) and from_f64.dtype == bool and (from_f64 == want).all()
    assert (utils_ground.segment_ground_pypatchworkpp(pts) == want).all()
    wide = torch.from_numpy(np.concatenate([pts, np.ones((len(pts), 2), np.float32)], axis=1)).to(DEV)     # [n, 5]: x, y, z first
    assert (utils_ground.segment_ground_pypatchworkpp(wide).cpu().numpy() == want).all()
    both = utils_ground.segment_ground(a, pts)
    assert (both == (want & utils_ground.segment_ground_thres(a, pts))).all() and both.sum() < want.sum()
    on_gpu = utils_ground.segment_ground(a, torch.from_numpy(pts).to(DEV))
    assert on_gpu.is_cuda and (on_gpu.cpu().numpy() == both).all()
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils_ground.segment_ground(a, torch.from_numpy(pts))


def test_run_sequences_with_patchwork(tmp_path):
    """A synthetic sequence file without a `nonground` key: ground = "patchwork" is reported as such and gives a finite table;
    "auto" is what no setting at all gives.  Both of those runs go through this change's _sequence_ground, so this shows that
    the default IS "auto", not that "auto" is what the parent commit did: that rests on the code -- the new branch is taken for
    "patchwork" only and the lines below it are the parent's, untouched -- and on the existing sequence tests, which set no
    `ground` and still pass."""
    from icp_flow_amd import frame_pairs, synthetic
    d = synthetic.make_sequence(seed=3, num_frames=3, n_objects=6, n_max=400)
    ng = d.pop("nonground")
    sd = (ng & (np.linalg.norm(d["scene_flow"], axis=1) > 0.5)).astype(np.int64)
    os.makedirs(os.path.join(tmp_path, "val"))
    path = os.path.join(tmp_path, "val", "seq.npz")
    np.savez(path, **d, sd_labels=sd, fb_labels=ng.astype(np.int64))

    def go(**extra):
        a = frame_pairs.default_args(max_points=1024, speed=1.67, cluster="dbscan", min_cluster_size=20, range_x=80.0, range_y=80.0, epsilon=0.8)
        a.num_frames, a.range_z, a.ground_slack, a.eval_ground, a.pose_source = 3, 0.0, 0.05, False, "ego_motion_gt"
        for k, v in extra.items():
            setattr(a, k, v)
        return frame_pairs.run_sequences(a, [path], DEV)

    plain, auto, patch = go(), go(ground="auto"), go(ground="patchwork")
    assert plain["ground"] == auto["ground"] == "threshold" and patch["ground"] == "patchwork+threshold"
    for name, m in plain["metrics"].items():
        o = auto["metrics"][name]
        assert (m.num, m.num_data) == (o.num, o.num_data) and np.array_equal(np.float64(m.epe_avg).tobytes(), np.float64(o.epe_avg).tobytes()), name
    assert patch["frame_pairs"] == 2 and patch["metrics"]["overall_0"].num > 0 and np.isfinite(patch["metrics"]["overall_0"].epe_avg)

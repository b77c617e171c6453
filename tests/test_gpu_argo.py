"""The Argoverse 2 path on the GPU: icpflow_seq_argo_sample against the numpy restatement (tests/argo_restatement.py) on the
shapes where the gather and the row split can go wrong, and -- through utils_loading.argo_sample, calculate_metrics and
run_sequences(dataset="argo") -- against the g15 fixtures, the reference's own dataset_argo / calculate_metrics run on the CPU
(tools/gen_golden_argo.py)."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import argo_restatement as ar         # noqa: E402
import seqeval_restatement as sr      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
BACKGROUND = (5, 8, 9, 13, 21, 22)
GUARD, F64_SENTINEL, I32_SENTINEL = 16, 777.25, -77
OUTPUTS = (("raw_points", 3, torch.float64), ("time_indice", 1, torch.int32), ("sd_labels", 1, torch.int32), ("fb_labels", 1, torch.int32),
           ("scene_flow", 3, torch.float64))


def enqueue(pc1, pc2, flow, classes, v1, v2, background=BACKGROUND):
    """icpflow_seq_argo_sample on numpy inputs, on the current stream, nothing waited for: every output pre-filled with a
    sentinel, between GUARD elements on either side.  -> what `collect` reads (the inputs stay referenced until then)"""
    from icp_flow_amd import _lib
    code = {np.dtype(np.float32): _lib.DTYPE_FLOAT32, np.dtype(np.float64): _lib.DTYPE_FLOAT64}
    keep = [G(pc1), G(pc2), G(flow), G(np.asarray(classes).astype(np.float64)), G(np.asarray(v1, np.int64)), G(np.asarray(v2, np.int64))]
    m1, m2 = len(v1), len(v2)
    m = m1 + m2
    bufs = {}
    for name, width, dt in OUTPUTS:
        bufs[name] = torch.full((m * width + 2 * GUARD,), F64_SENTINEL if dt == torch.float64 else I32_SENTINEL, dtype=dt, device=DEV)
    bad = torch.full((3,), -5, dtype=torch.int64, device=DEV)
    bg = np.asarray(background, np.int32)
    at = lambda t, k: ctypes_ptr(t.data_ptr() + k * t.element_size())   # noqa: E731
    _lib.call("icpflow_seq_argo_sample", _lib.ptr(keep[0]), len(pc1), _lib.ptr(keep[1]), len(pc2), code[pc1.dtype], _lib.ptr(keep[2]),
              code[flow.dtype], _lib.ptr(keep[3]), _lib.ptr(keep[4]), m1, _lib.ptr(keep[5]), m2, ctypes_ptr(bg.ctypes.data), len(bg),
              float(ar.sd_threshold(flow.dtype)), *[at(bufs[name], GUARD) for name, _, _ in OUTPUTS], at(bad, 1), _lib.stream(DEV))
    return dict(bufs=bufs, bad=bad, m=m, keep=keep)


def ctypes_ptr(address):
    import ctypes
    return ctypes.c_void_p(address)


def collect(job):
    """-> (outputs as numpy arrays, bad rows); the guards around every output must be untouched"""
    torch.cuda.synchronize()
    out, m = {}, job["m"]
    for name, width, dt in OUTPUTS:
        host = job["bufs"][name].cpu().numpy()
        sentinel = F64_SENTINEL if dt == torch.float64 else I32_SENTINEL
        assert (host[:GUARD] == sentinel).all() and (host[GUARD + m * width:] == sentinel).all(), f"{name}: a guard element was written"
        body = host[GUARD:GUARD + m * width]
        out[name] = body.reshape(m, 3) if width == 3 else body
    bad = job["bad"].cpu().numpy()
    assert bad[0] == -5 and bad[2] == -5
    return out, int(bad[1])


def make_inputs(n1, n2, m1, m2, ptype, ftype, class_type, order, seed):
    """A file's arrays with every row that no index selects NaN (int8 classes: 99).  Flow norms on both sides of 0.05, a few
    selected rows with a NaN flow, and with float32 classes a few NaN classes (IEEE: sd = 0, fb = 1)."""
    rng = np.random.default_rng(seed)

    def indices(n, m):
        if m > n or order == "repeats":
            return rng.integers(0, max(n, 1), size=m) if n else np.zeros(0, np.int64)
        v = rng.choice(n, size=m, replace=False)
        return np.sort(v) if order == "sorted" else v

    v1, v2 = indices(n1, m1), indices(n2, m2)
    pc1, pc2, flow = np.full((n1, 3), np.nan, ptype), np.full((n2, 3), np.nan, ptype), np.full((n1, 3), np.nan, ftype)
    pc1[v1], pc2[v2] = rng.uniform(-50, 50, size=(m1, 3)).astype(ptype), rng.uniform(-50, 50, size=(m2, 3)).astype(ptype)
    d = rng.normal(size=(n1, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    every = (d * np.where(rng.random(n1) < 0.5, rng.uniform(0.0, 0.0499, n1), rng.uniform(0.0501, 2.0, n1))[:, None]).astype(ftype)
    every[3::17] = np.nan
    flow[v1] = every[v1]
    values = np.array(list(BACKGROUND) + [-1, 0, 1, 7, 17, 30])
    drawn = values[rng.integers(0, len(values), size=n1)]
    if class_type == np.int8:
        classes = np.full(n1, 99, np.int8)
        classes[v1] = drawn[v1]
    else:
        classes = np.full(n1, np.nan, np.float32)
        classes[v1] = np.where(np.arange(n1) % 13 == 5, np.nan, drawn)[v1]
    return pc1, pc2, flow, classes, v1, v2


def same(got, want):
    for k in ar.SAMPLE_KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k], equal_nan=True), k


SHAPES = [(1, 1, 1, 1), (5, 3, 0, 3), (5, 3, 5, 0), (0, 0, 0, 0), (64, 64, 63, 65), (257, 300, 257, 1), (1000, 1000, 777, 1023)]


@pytest.mark.parametrize("ptype,ftype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)],
                         ids=["p32f32", "p32f64", "p64f32", "p64f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_equals_the_restatement(shape, ptype, ftype):
    """Every output array_equal (NaN flows are gathered as NaN), guards untouched, no bad row; index lists sorted, shuffled
    and with repeats (m2 > n2 in two shapes), classes from int8 and from float32, every unselected row NaN."""
    n1, n2, m1, m2 = shape
    for k, (class_type, order) in enumerate(((np.int8, "sorted"), (np.float32, "shuffled"), (np.float32, "repeats"))):
        pc1, pc2, flow, classes, v1, v2 = make_inputs(n1, n2, m1, m2, ptype, ftype, class_type, order, seed=1000 * n1 + 10 * m2 + k)
        got, bad = collect(enqueue(pc1, pc2, flow, classes, v1, v2))
        assert bad == 0
        same(got, ar.sample(pc1, pc2, flow, classes, v1, v2, BACKGROUND))
        if m1 >= 63:
            rows = got["time_indice"] == 1
            assert 0 < got["sd_labels"][rows].sum() < m1 and 0 < got["fb_labels"][rows].sum() < m1
            assert np.isnan(got["scene_flow"]).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_straddling_rows_get_numpys_labels(dtype):
    """The rows of tests/test_argo.py's order test: the two association orders of the norm give different labels on every
    one of them; the kernel's are np.linalg.norm's."""
    from icp_flow_amd import utils_loading
    rows = ar.straddling_rows(dtype)
    n = len(rows)
    assert n >= 1000
    want = np.linalg.norm(rows, axis=-1) > (0.5 * 0.1)
    got = utils_loading.argo_sample(rows.astype(np.float32), np.zeros((0, 3), np.float32), rows, np.zeros(n, np.int8), np.arange(n), np.arange(0))
    assert got["sd_labels"].dtype == torch.int32 and got["raw_points"].dtype == torch.float32
    assert np.array_equal(got["sd_labels"].cpu().numpy(), want.astype(np.int32))
    assert np.array_equal(got["scene_flow"].cpu().numpy(), rows.astype(np.float64)) and bool((got["fb_labels"] == 1).all())


def test_indices_outside_their_cloud_are_counted_and_not_written():
    from icp_flow_amd import utils_loading
    n1, n2 = 200, 150
    pc1, pc2, flow, classes, v1, v2 = make_inputs(n1, n2, 130, 140, np.float32, np.float32, np.int8, "shuffled", seed=3)
    v1, v2 = v1.astype(np.int64), v2.astype(np.int64)
    bad1, bad2 = np.array([0, 64, 129]), np.array([5, 63, 139])
    v1[bad1] = (-1, n1, 1 << 40)
    v2[bad2] = (1 << 40, -1, n2)
    got, bad = collect(enqueue(pc1, pc2, flow, classes, v1, v2))
    assert bad == 6
    bad_rows = np.concatenate([bad2, len(v2) + bad1])
    for name, _, dt in OUTPUTS:
        assert (got[name][bad_rows] == (F64_SENTINEL if dt == torch.float64 else I32_SENTINEL)).all(), name
    good1, good2 = np.setdiff1d(np.arange(len(v1)), bad1), np.setdiff1d(np.arange(len(v2)), bad2)
    want = ar.sample(pc1, pc2, flow, classes, v1[good1], v2[good2], BACKGROUND)
    good = np.concatenate([good2, len(v2) + good1])
    same({k: got[k][good] for k in ar.SAMPLE_KEYS}, want)
    with pytest.raises(IndexError, match="6 of 270"):
        utils_loading.argo_sample(pc1, pc2, flow, classes, v1, v2)
    with pytest.raises(IndexError, match="boolean mask"):
        utils_loading.argo_sample(pc1, pc2, flow, classes, np.ones(n1 + 1, bool), v2[good2])
    # a boolean mask is np.flatnonzero on the host; device tensors are taken where they are
    mask = np.zeros(n1, bool)
    mask[v1[good1]] = True
    by_mask = utils_loading.argo_sample(G(pc1), G(pc2), G(flow), G(classes), mask, G(v2[good2]))
    want = ar.sample(pc1, pc2, flow, classes, mask, v2[good2], BACKGROUND)
    assert by_mask["raw_points"].is_cuda and by_mask["raw_points"].dtype == torch.float32
    same({k: by_mask[k].cpu().numpy().astype(want[k].dtype) for k in ar.SAMPLE_KEYS}, want)


def _same_meters(got, ref):
    from icp_flow_amd import utils_eval
    assert list(got) == list(ref)
    for name in got:
        assert got[name].num == ref[name].num and got[name].num_data == ref[name].num_data, name
        for m in utils_eval.METRIC_NAMES:
            for field in ("_sum", "_avg", "_data"):
                a, b = np.asarray(getattr(got[name], m + field), np.float64), np.asarray(getattr(ref[name], m + field), np.float64)
                assert np.array_equal(a, b, equal_nan=True), (name, m, field)


@pytest.fixture(scope="module")
def demo():
    """the real sample in file form (g8_demo's rows scattered into 90 000-row arrays, NaN elsewhere) and its sample on the device"""
    from icp_flow_amd import utils_loading
    arrays, pred = ar.file_arrays(ar.DEMO)
    data = utils_loading.argo_sample(arrays["pc1"], arrays["pc2"], arrays["gt_flow_0_1"], arrays["pc1_classes"],
                                     arrays["pc1_flows_valid_idx"], arrays["pc2_flows_valid_idx"])
    return dict(arrays=arrays, pred=pred, data=data)


def test_demo_sample_labels_equal_the_reference(demo):
    want = ar.recorded_sample(ar.DEMO)
    data = demo["data"]
    assert data["raw_points"].dtype == torch.float32 and data["scene_flow"].dtype == torch.float64
    for k in ar.SAMPLE_KEYS:
        assert np.array_equal(data[k].cpu().numpy(), want[k]), k
    rows = want["time_indice"] == 1
    sd, fb = data["sd_labels"].cpu().numpy()[rows] == 1, data["fb_labels"].cpu().numpy()[rows] == 1
    assert (int(sd.sum()), int((sd & fb).sum()), int((~sd & fb).sum())) == (4250, 4250, 414)


@pytest.mark.parametrize("setting", list(ar.SETTINGS))
def test_demo_sample_table_against_the_reference(demo, setting):
    """calculate_metrics on the device-built sample with g8's flow: every count exactly the reference's, every meter within
    the bound tests/test_gpu_seqeval.py asserts for G13 -- 2 n 2^-53 relative for the mean error (any summation order against
    numpy's; the ground truth is the file's own here, so its term is zero), fractions equal as float32."""
    from icp_flow_amd import utils_eval
    args, rec = ar.setting_args(setting), ar.Recorded(ar.load(ar.DEMO), setting)
    pred = G(demo["pred"])
    table, esum, kept0, outside = utils_eval.sequence_table(args, demo["data"], pred)
    want, want_epe, want_kept0 = sr.reference_table(rec, 0)
    counts = table.copy()
    counts[:, :, 1] = 0
    assert np.array_equal(counts, want) and kept0 == want_kept0 and outside == 0
    bound = lambda value, n: 2 * n * sr.U * value      # noqa: E731
    for j in range(2):
        for c in range(6):
            n = int(table[j, c, 0])
            if n and not np.isnan(want_epe[j, c]):
                got = esum[j, c] / n
                print(f"demo {setting} row {j} class {c}: n {n}, mean e {got!r} vs {want_epe[j, c]!r}")
                assert abs(got - want_epe[j, c]) <= bound(want_epe[j, c], n)
    meters = utils_eval.calculate_metrics(args, demo["data"], pred, utils_eval.new_metric_table(2))
    sr.check_meters(meters, rec, 0, bound)


@pytest.fixture(scope="module")
def argo_dir(tmp_path_factory, demo):
    """a directory with the demo sample in file form and one synthetic file (clustered objects, so that DBSCAN finds segments)"""
    from icp_flow_amd import synthetic
    tmp = str(tmp_path_factory.mktemp("argo"))
    np.savez(os.path.join(tmp, "a_demo.npz"), **demo["arrays"])
    d = synthetic.make_frame_pair(seed=12, n_objects=6, n_min=600, n_max=1500, n_background=600)
    rng = np.random.default_rng(16)
    n, m1, m2 = 7000, len(d["points_src"]), len(d["points_dst"])
    v1, keep2 = rng.permutation(n)[:m1], np.zeros(n, bool)       # an unsorted index list and a boolean mask
    keep2[rng.choice(n, m2, replace=False)] = True
    pc1, pc2, flow = (np.full((n, 3), np.nan, np.float32) for _ in range(3))
    classes = np.full(n, 99, np.int8)
    pc1[v1], pc2[keep2], flow[v1] = d["points_src"], d["points_dst"], d["gt_flow"]
    classes[v1] = np.array(list(BACKGROUND) + [-1, 0, 18, 18, 18, 16])[rng.integers(0, 12, size=m1)]
    np.savez(os.path.join(tmp, "b_synthetic.npz"), pc1=pc1, pc2=pc2, gt_flow_0_1=flow, pc1_classes=classes, pc1_flows_valid_idx=v1,
             pc2_flows_valid_idx=keep2)
    return tmp


def test_run_sequences_end_to_end(argo_dir, monkeypatch, capsys):
    """run_sequences(dataset="argo"), DBSCAN, main.sh:38's ranges, if_verbose: each file's flow is register_frame_pair's on
    load_frame_pair's frame pair, the table is calculate_metrics on the restated samples with those flows bit for bit, each
    report's segments sum to its frame's row, and the command line prints the same 18 table lines."""
    from icp_flow_amd import frame_pairs, utils_eval
    paths = frame_pairs.list_frame_pairs(argo_dir)
    assert len(paths) == 2 and all(frame_pairs.is_argo(p) for p in paths)
    a = frame_pairs.default_args(cluster="dbscan", speed=1.67)
    for k, v in dict(ar.SETTINGS["argo"], num_frames=2, ground="patchwork", if_verbose=True).items():
        setattr(a, k, v)
    flows, real = [], frame_pairs.register_frame_pair

    def spy(args, fp, device, gap=None):
        out = real(args, fp, device, gap)
        flows.append(out["flow"])
        return out

    monkeypatch.setattr(frame_pairs, "register_frame_pair", spy)
    with contextlib.redirect_stdout(io.StringIO()) as text:
        res = frame_pairs.run_sequences(a, paths, DEV, dataset="argo")
    monkeypatch.undo()
    assert res["sequences"] == 2 and res["frame_pairs"] == 2 and res["ground"] == "none" and len(flows) == 2
    want = utils_eval.new_metric_table(2)
    for path, flow in zip(paths, flows):
        fp = frame_pairs.load_frame_pair(path)
        assert fp.gap == 1 and np.array_equal(fp.pose_exact, np.eye(4))
        direct = frame_pairs.register_frame_pair(a, fp, DEV)
        assert direct["translation_frame"] == 2 * 1.67 and torch.equal(direct["flow"], flow)
        with np.load(path) as z:
            s = ar.sample(z["pc1"], z["pc2"], z["gt_flow_0_1"], z["pc1_classes"], z["pc1_flows_valid_idx"], z["pc2_flows_valid_idx"], BACKGROUND)
        s["raw_points"] = s["raw_points"].astype(np.float32)
        m2 = len(fp.points_dst)
        assert len(s["time_indice"]) == m2 + len(flow)
        flow_seq = np.concatenate([np.zeros((m2, 3), np.float32), flow.cpu().numpy()])
        with contextlib.redirect_stdout(io.StringIO()):
            utils_eval.calculate_metrics(a, s, flow_seq, want)
    _same_meters(res["metrics"], want)
    assert res["metrics"]["dynamic_fg_0"].num > 0 and res["metrics"]["static_bg_0"].num > 0 and res["metrics"]["overall_0"].epe_avg < 0.5
    # the verbose loop: row 8's own property, per file
    reports = res["segments"]
    assert [r["gap"] for r in reports] == [1, 1] and [r["sequence"] for r in reports] == paths
    for rep in reports:
        seg, frame = rep["segments"], rep["frame"]["overall"]
        n = frame[5]
        assert n > 0 and int(seg.n.sum()) == n
        with np.errstate(all="ignore"):
            counts = [int(np.nan_to_num(np.round(getattr(seg, k).astype(np.float64) * seg.n)).sum()) for k in ("accs", "accr", "outlier", "routlier")]
        assert counts == [int(round(float(frame[1 + k]) * n)) for k in range(4)]
    assert "debug frame: 1/2,  overall, EPE: " in text.getvalue() and "eval segment:" in text.getvalue()
    # the command line, without the verbose loop: the same table
    frame_pairs.main([argo_dir, "--protocol", "reference", "--dataset", "argo", "--cluster", "dbscan", "--speed", "1.67", "--range-x", "10000",
                      "--range-y", "10000", "--range-z", "-10000", "--ground-slack", "0"])
    printed = capsys.readouterr().out.split("\n")
    table = utils_eval.format_metric_table(res["metrics"], 2).split("\n")
    assert len(table) == 1 + 18
    start = printed.index(table[0])
    assert printed[start:start + 19] == table


def test_reruns_and_two_streams_are_bit_identical():
    """The same call twice, and two different samples enqueued on two streams before either is waited for, against the same
    two one after the other on one stream."""
    cases = [make_inputs(1000, 900, 777, 1023, np.float32, np.float32, np.float32, "shuffled", seed=61),
             make_inputs(3000, 2500, 2900, 2100, np.float64, np.float64, np.int8, "sorted", seed=62)]
    first = [collect(enqueue(*c))[0] for c in cases]
    again = [collect(enqueue(*c))[0] for c in cases]
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    jobs = []
    torch.cuda.synchronize()
    for c, s in zip(cases, streams):
        with torch.cuda.stream(s):
            jobs.append(enqueue(*c))
    both = [collect(j)[0] for j in jobs]
    for a, b, c in zip(first, again, both):
        for k in ar.SAMPLE_KEYS:
            assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_an_empty_sample_succeeds():
    from icp_flow_amd import utils_loading
    e3, e1 = np.zeros((0, 3), np.float64), np.zeros(0, np.int64)
    got = utils_loading.argo_sample(e3, e3, e3.astype(np.float32), e1, e1, e1)
    assert got["raw_points"].shape == (0, 3) and got["time_indice"].shape == (0,) and got["scene_flow"].dtype == torch.float64

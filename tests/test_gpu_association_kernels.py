"""The device-side association (csrc/assoc.hip: icpflow_assoc_assign, icpflow_assoc_collect) and its two neighbours in the chain
match_pcds enqueues (icpflow_gather_segments in front of a stage, icpflow_flow_rigid_rows behind the pair rows; with them
icpflow_transform_points), called one kernel at a time through the C ABI.

The association and the gather are compared with `array_equal` against tests/assoc_restatement.py (pinned to the reference's
loop by tests/test_association_restatement.py) and numpy indexing: no tolerance.  The flow and the transform are compared with
an fp64 evaluation under bounds derived from the kernels' rounding count (docstrings below).  Every output is poisoned first and
sits between guard words."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assoc_restatement as ar         # noqa: E402
from icp_flow_amd import _lib          # noqa: E402

DEV = torch.device("cuda:0")
F = np.float32
GUARD, POISON = 256, 0xA5              # bytes of guard on either side of an output; the byte that outputs and guards start as
E_ARG, E_LIMIT = -1, -3
U = 2.0 ** -24                         # unit roundoff of float32


class Out:
    """A device array filled with POISON bytes between two guards."""

    def __init__(self, shape, dtype, fill=None):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.raw = torch.full((self.n + 2 * GUARD,), POISON, dtype=torch.uint8, device=DEV)
        if fill is not None:
            h = np.ascontiguousarray(fill, self.dtype).reshape(-1).view(np.uint8)
            assert h.size == self.n
            self.raw[GUARD:GUARD + self.n] = torch.from_numpy(h.copy()).to(DEV)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.raw.data_ptr() + GUARD)

    def _host(self):
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == POISON).all() and (h[GUARD + self.n:] == POISON).all(), "a guard word was overwritten"
        return h[GUARD:GUARD + self.n]

    def read(self):
        return self._host().view(self.dtype).reshape(self.shape).copy()

    def untouched(self):
        return bool((self._host() == POISON).all())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gpu_assign(st, nxt=None, seg2=None, params=ar.PARAMS):
    """icpflow_assoc_assign of stage `st` -> best [S] (and, with the next stage's candidates, active2 [K2], seg2 [2,3,K2])."""
    r, si, di, act = dev(st.result), dev(st.si), dev(st.di), dev(st.active)
    best = Out((st.S,), np.int32)
    K2, si2, di2, segd, act2 = 0, None, None, None, None
    if nxt is not None:
        K2, si2, di2 = nxt.K, dev(nxt.si), dev(nxt.di)
        segd, act2 = Out((2, 3, K2), np.int64, fill=seg2), Out((K2,), np.uint8)
    _lib.call("icpflow_assoc_assign", _lib.ptr(r), _lib.ptr(si), _lib.ptr(di), st.K, _lib.ptr(act), st.S, st.D, float(params.tf),
              float(params.thres_iou), float(params.rot_limit), float(params.thres_error), best.ptr, K2, _lib.ptr(si2),
              _lib.ptr(di2), segd.ptr if segd else None, act2.ptr if act2 else None, _lib.stream(DEV))
    if nxt is None:
        return best.read()
    return best.read(), act2.read(), segd.read()


def want_assign(st):
    return ar.assign(ar.PARAMS, st.S, st.D, st.si, st.di, st.active, st.result)


# ------------------------------------------------------------------------------------------------ icpflow_assoc_assign
def test_assign_equals_the_restatement_on_random_stages():
    """S, D in 1 ... 40, ties, NaNs in every array, infinite errors, threshold values, every kind of mask -- and the run enters
    every branch of the statement (tests/assoc_restatement.py: Branches.check)."""
    rng = np.random.default_rng(20261019)
    seen = ar.Branches()
    for trial in range(200):
        S, D = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        mode, active = ar.stage_plan(trial)
        st = ar.random_stage(rng, S, D, mode=mode, active=active)
        got, want = gpu_assign(st), want_assign(st)
        assert np.array_equal(got, want), (trial, S, D, st.K)
        if active == "zeros":
            assert (got == -1).all()
        seen.count(ar.PARAMS, st, want)
    print(seen)
    seen.check()


FIXED = [  # S, D, K, layout
    (1, 1, 1, "random"), (37, 29, 1, "random"),                                   # rows without a candidate: -1
    (32, 33, 1023, "random"), (32, 33, 1024, "random"), (32, 33, 1025, "random"), (71, 71, 5000, "random"),   # strided loops
    (1024, 1024, 1024, "diagonal"), (1024, 1024, 3000, "random"), (1024, 1, 1024, "random"), (1, 1024, 1024, "random"),
]


@pytest.mark.parametrize("S,D,K,layout", FIXED)
def test_assign_fixed_shapes(S, D, K, layout):
    rng = np.random.default_rng(S * 7919 + D * 31 + K)
    if layout == "diagonal":
        order = rng.permutation(K).astype(np.int32)
        cells = (order, order.copy())
    else:
        cells = ar.random_cells(rng, S, D, K)
    has = np.zeros(S, bool)
    has[cells[0]] = True
    for active in (None, "ones", "random", "zeros"):
        st = ar.random_stage(rng, S, D, cells=cells, active=active)
        got, want = gpu_assign(st), want_assign(st)
        assert got.shape == (S,) and np.array_equal(got, want), active
        assert (got[~has] == -1).all()
        if active == "zeros":
            assert (got == -1).all()
        elif active != "random":
            assert (got >= 0).any() or K == 1 or S == 1     # (one row with a thousand candidates: a kept NaN error un-matches it)


def test_tie_rule_built_by_hand():
    """Three kept candidates of one source row with equal error, destination rows 7, 3, 5 in that order -> the one at row 3; a
    smaller error that fails a reject test and a smaller error that is inactive do not count."""
    si = [1, 1, 1, 1, 1, 0, 3]
    di = [7, 3, 5, 1, 0, 2, 7]
    st = ar.plain_stage(4, 8, si, di)
    f = ar.unpack(st.result, st.K)
    f.errors[3] = f.errors[4] = F(0.05)
    f.ious[3] = (F(0.9), F(0.1))                  # fails min(iou) >= thres_iou
    st.active = np.array([1, 1, 1, 1, 0, 1, 1], np.uint8)
    want = np.array([5, 1, -1, 6], np.int32)
    assert np.array_equal(want_assign(st), want)
    assert np.array_equal(gpu_assign(st), want)
    # ... and the same row's equal errors on both sides of index 1024 in candidate order (two trips of a thread's loop)
    S = D = 40
    filler = [(s, d) for s in range(S) if s != 20 for d in range(D)][:1098]
    cand = filler[:1000] + [(20, 9)] + filler[1000:1049] + [(20, 4)] + filler[1049:]
    assert len(cand) == 1100 and cand[1000] == (20, 9) and cand[1050] == (20, 4)
    st = ar.plain_stage(S, D, [c[0] for c in cand], [c[1] for c in cand])
    want = want_assign(st)
    assert want[20] == 1050
    assert np.array_equal(gpu_assign(st), want)
    # reversed: the later candidate has the larger destination row
    cand[1000], cand[1050] = cand[1050], cand[1000]
    st = ar.plain_stage(S, D, [c[0] for c in cand], [c[1] for c in cand])
    want = want_assign(st)
    assert want[20] == 1000
    assert np.array_equal(gpu_assign(st), want)


def _distinct_seg(K2):
    return (1000 + np.arange(6 * K2, dtype=np.int64)).reshape(2, 3, K2)      # six distinct values per candidate: a stray write shows


@pytest.mark.parametrize("S,D,K1,K2", [(40, 40, 150, 1300), (40, 37, 60, 1025), (12, 9, 20, 30)])
def test_two_stages_switch_and_second_assign(S, D, K1, K2):
    rng = np.random.default_rng(K2)
    st1 = ar.random_stage(rng, S, D, K=K1, active=None, nan_rate=0.005)
    st2 = ar.random_stage(rng, S, D, K=K2, active="ones")
    seg2 = _distinct_seg(K2)
    best1, act2, seg_got = gpu_assign(st1, nxt=st2, seg2=seg2)
    want1 = want_assign(st1)
    want_act, want_seg = ar.switch(want1, st1.si, st1.di, D, st2.si, st2.di, seg2)
    assert (want1 >= 0).sum() >= 2 and 0 < want_act.sum() < K2            # the case switches some off and leaves some on
    assert np.array_equal(best1, want1)
    assert np.array_equal(act2, want_act)
    assert np.array_equal(seg_got, want_seg)
    assert (seg_got[:, 1, :][:, want_act == 0] == 0).all() and np.array_equal(seg_got[:, [0, 2], :], seg2[:, [0, 2], :])
    st2.active = act2
    assert np.array_equal(gpu_assign(st2), want_assign(st2))


def test_switch_of_a_single_candidate():
    """K2 = 1: off through its source row, off through its destination row, on."""
    st1 = ar.plain_stage(5, 5, [0, 1], [0, 2])                       # matches rows 0 -> 0 and 1 -> 2
    assert np.array_equal(want_assign(st1), [0, 1, -1, -1, -1])
    for s2, d2, on in ((0, 4, 0), (3, 2, 0), (3, 4, 1), (1, 0, 0)):
        st2 = ar.plain_stage(5, 5, [s2], [d2])
        seg2 = _distinct_seg(1)
        best1, act2, seg_got = gpu_assign(st1, nxt=st2, seg2=seg2)
        want_act, want_seg = ar.switch(best1, st1.si, st1.di, 5, st2.si, st2.di, seg2)
        assert int(want_act[0]) == on
        assert np.array_equal(act2, want_act) and np.array_equal(seg_got, want_seg), (s2, d2)


# ----------------------------------------------------------------------------------------------- icpflow_assoc_collect
def gpu_collect(best1, st1, best2, st2, src_table, dst_table, stride, S, cap):
    h = [dev(np.asarray(best1, np.int32)), dev(st1.result), dev(st1.si), dev(st1.di)]
    h2 = [dev(np.asarray(best2, np.int32)), dev(st2.result), dev(st2.si), dev(st2.di)] if st2 is not None else [None] * 4
    ts, td = dev(src_table), dev(dst_table)
    rows, T, count = Out((cap, 10), F), Out((cap, 16), F), Out((1,), np.int32)
    _lib.call("icpflow_assoc_collect", *[_lib.ptr(x) for x in h], st1.K, *[_lib.ptr(x) for x in h2], st2.K if st2 is not None else 0,
              _lib.ptr(ts), _lib.ptr(td), stride, S, cap, rows.ptr, T.ptr, count.ptr, _lib.stream(DEV))
    return rows.read(), T.read(), int(count.read()[0])


def _label_table(rng, n, stride):
    """float64 [n, stride], the label in column 0: negative, fractional and large labels (the float32 cast is part of the
    statement), junk in the other columns."""
    special = np.array([-2.5, 0.1, 16777217.0, 1.0e30, -1.0e8, 123456789.0, 0.0, 1.0 / 3.0])
    lab = rng.permutation(np.concatenate([special, 10.0 + np.arange(max(n - len(special), 0))]))[:n]
    table = rng.normal(0, 1e6, (n, stride))
    table[:, 0] = lab
    return table


def _check_collect(best1, st1, best2, st2, stride, S, D, cap, rng):
    ts, td = _label_table(rng, S, stride), _label_table(rng, D, stride)
    rows, T, count = gpu_collect(best1, st1, best2, st2, ts, td, stride, S, cap)
    two = (st2.si, st2.di, st2.result) if st2 is not None else None
    want_rows, want_T, want_count = ar.collect(best1, (st1.si, st1.di, st1.result), best2, two, ts[:, 0], td[:, 0], cap)
    assert count == want_count, (count, want_count, cap)
    assert np.array_equal(bits(rows), bits(want_rows)), cap
    assert np.array_equal(bits(T), bits(want_T)), cap
    return count


@pytest.mark.parametrize("stride", [1, 9])
def test_collect_equals_the_restatement(stride):
    rng = np.random.default_rng(stride)
    S, D = 30, 26
    st1 = ar.random_stage(rng, S, D, K=90, active=None, nan_rate=0.005)
    st2 = ar.random_stage(rng, S, D, K=200, active="ones", nan_rate=0.005)
    best1 = want_assign(st1)
    st2.active, _ = ar.switch(best1, st1.si, st1.di, D, st2.si, st2.di, _distinct_seg(st2.K))
    best2 = want_assign(st2)
    P1, P = int((best1 >= 0).sum()), int((best1 >= 0).sum() + (best2 >= 0).sum())
    assert P1 >= 3 and P - P1 >= 3
    for cap in (2 * S, P, P - 1, 1, P + 1, P1, P1 + 1):
        count = _check_collect(best1, st1, best2, st2, stride, S, D, cap, rng)
        assert count == min(P, cap)
    for cap in (2 * S, P1, P1 - 1, 1, P1 + 1):                         # stage 2 absent: K2 = 0, NULL pointers
        assert _check_collect(best1, st1, None, None, stride, S, D, cap, rng) == min(P1, cap)
    # no match at all: every row is filler
    none = np.full(S, -1, np.int32)
    assert _check_collect(none, st1, none, st2, stride, S, D, 2 * S, rng) == 0
    assert _check_collect(none, st1, None, None, stride, S, D, 3, rng) == 0
    # an abandoned batch in stage 1, in stage 2, in both: count = -1 (the rows are written all the same)
    for neg1, neg2 in ((True, False), (False, True), (True, True)):
        a, b = (ar.random_stage(rng, S, D, K=90, active=None, iters=-1 if neg1 else 3),
                ar.random_stage(rng, S, D, K=200, active="ones", iters=-1 if neg2 else 0))
        assert _check_collect(want_assign(a), a, want_assign(b), b, stride, S, D, 2 * S, rng) == -1
    a = ar.random_stage(rng, S, D, K=90, active=None, iters=-(2 ** 31))
    assert _check_collect(want_assign(a), a, None, None, stride, S, D, 2 * S, rng) == -1


def test_collect_at_the_row_limit():
    """S = D = 1024: 2 S flags, two trips of every loop of the kernel."""
    rng = np.random.default_rng(1024)
    S = D = 1024
    st1 = ar.random_stage(rng, S, D, cells=ar.random_cells(rng, S, D, 3000), active=None, nan_rate=0.002)
    st2 = ar.random_stage(rng, S, D, cells=ar.random_cells(rng, S, D, 2500), active="ones", nan_rate=0.002)
    best1, best2 = want_assign(st1), want_assign(st2)
    P = int((best1 >= 0).sum() + (best2 >= 0).sum())
    assert P > 1024
    for cap in (2 * S, P, 1025):
        assert _check_collect(best1, st1, best2, st2, 9, S, D, cap, rng) == min(P, cap)


# ------------------------------------------------------------------------------------------------------------ refusals
def _refused(name, args, code, outs):
    rc = getattr(_lib._L, name)(*args)
    msg = (_lib._L.icpflow_last_error() or b"").decode()
    assert rc == code and name in msg, (rc, msg)
    for o in outs:
        assert o.untouched(), msg


def test_refusals_come_before_any_launch():
    rng = np.random.default_rng(3)
    st = ar.random_stage(rng, 8, 8, K=20, active=None)
    r, si, di = dev(st.result), dev(st.si), dev(st.di)
    best, seg2, act2 = Out((1025,), np.int32), Out((2, 3, 20), np.int64), Out((20,), np.uint8)
    p, q = ar.PARAMS, _lib.ptr
    th = (float(p.tf), float(p.thres_iou), float(p.rot_limit), float(p.thres_error))
    stream = _lib.stream(DEV)

    def assign(K=20, S=8, D=8, d_best=best.ptr, K2=0, si2=None, di2=None, s2=None, a2=None):
        return (q(r), q(si), q(di), K, None, S, D, *th, d_best, K2, si2, di2, s2, a2, stream)

    outs = (best, seg2, act2)
    _refused("icpflow_assoc_assign", assign(S=1025), E_LIMIT, outs)
    _refused("icpflow_assoc_assign", assign(D=1025), E_LIMIT, outs)
    _refused("icpflow_assoc_assign", assign(K=0), E_LIMIT, outs)
    _refused("icpflow_assoc_assign", assign(d_best=None), E_ARG, outs)
    full = dict(si2=q(si), di2=q(di), s2=seg2.ptr, a2=act2.ptr)
    for missing in full:
        _refused("icpflow_assoc_assign", assign(K2=20, **{**full, missing: None}), E_ARG, outs)
    _refused("icpflow_assoc_assign", assign(K2=-1, **full), E_ARG, outs)

    b1 = dev(np.full(8, -1, np.int32))
    table = dev(np.arange(8, dtype=np.float64))
    rows, T, count = Out((16, 10), F), Out((16, 16), F), Out((1,), np.int32)

    def collect(S=8, cap=16, stride=1, K2=0, two=(None, None, None, None)):
        return (q(b1), q(r), q(si), q(di), 20, *two, K2, q(table), q(table), stride, S, cap, rows.ptr, T.ptr, count.ptr, stream)

    outs = (rows, T, count)
    _refused("icpflow_assoc_collect", collect(cap=0), E_LIMIT, outs)
    _refused("icpflow_assoc_collect", collect(stride=0), E_LIMIT, outs)
    _refused("icpflow_assoc_collect", collect(S=1025), E_LIMIT, outs)
    full = [q(b1), q(r), q(si), q(di)]
    for missing in range(4):
        _refused("icpflow_assoc_collect", collect(K2=20, two=[None if i == missing else x for i, x in enumerate(full)]), E_ARG, outs)
    _refused("icpflow_assoc_collect", collect(K2=-1, two=full), E_ARG, outs)


# -------------------------------------------------------------------------------------------------- reruns and streams
def test_reruns_and_another_stream_give_identical_bits():
    rng = np.random.default_rng(11)
    S = D = 1024
    st1 = ar.random_stage(rng, S, D, cells=ar.random_cells(rng, S, D, 5000), active="random")
    st2 = ar.random_stage(rng, S, D, cells=ar.random_cells(rng, S, D, 3000), active="ones")
    seg2 = _distinct_seg(st2.K)
    first = gpu_assign(st1, nxt=st2, seg2=seg2)
    want = want_assign(st1)
    assert np.array_equal(first[0], want) and np.array_equal(first[1], ar.switch(want, st1.si, st1.di, D, st2.si, st2.di, seg2)[0])
    for _ in range(2):
        again = gpu_assign(st1, nxt=st2, seg2=seg2)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = gpu_assign(st1, nxt=st2, seg2=seg2)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------------ icpflow_flow_rigid_rows
def gpu_flow(pts, labels, pair_rows, stride, T, P, pose):
    N = len(pts)
    d = [dev(pts), dev(labels), dev(pair_rows) if P > 0 else None, dev(T) if P > 0 else None, dev(pose)]
    flow = Out((N, 3), F)
    _lib.call("icpflow_flow_rigid_rows", _lib.ptr(d[0]), _lib.ptr(d[1]), N, _lib.ptr(d[2]), stride, _lib.ptr(d[3]), P,
              _lib.ptr(d[4]), flow.ptr, _lib.stream(DEV))
    return flow.read()


def lookup(labels, pair_labels):
    """Per point the LAST pair that lists its label (the reference's loop assigns them in order), or -1."""
    idx = np.full(len(labels), -1, np.int64)
    with np.errstate(invalid="ignore"):
        for p in range(len(pair_labels)):
            idx[labels == pair_labels[p]] = p                       # (== : -0.0 matches 0.0, a NaN matches nothing)
    return idx


def exact_flow(pts, idx, T, pose, shift=0):
    """utils_flow.py:57-69 in fp64: -> flow [N,3] and the bound's magnitude (|T| |pose| p~)_r + |p_r| [N,3]; `shift` looks one
    pair aside."""
    N, P = len(pts), len(T)
    matched = idx >= 0
    Tp = np.tile(np.eye(4), (N, 1, 1))
    if matched.any():
        Tp[matched] = np.asarray(T, np.float64).reshape(P, 4, 4)[np.clip(idx[matched] + shift, 0, P - 1)]
    ph = np.concatenate([pts.astype(np.float64), np.ones((N, 1))], axis=1)
    M = Tp @ pose.astype(np.float64)
    flow = np.einsum("nij,nj->ni", M, ph)[:, :3] - ph[:, :3]
    mag = np.einsum("nij,nj->ni", np.abs(Tp) @ np.abs(pose.astype(np.float64)), np.abs(ph))[:, :3] + np.abs(ph[:, :3])
    return flow, mag


def _rigid(rng, n, scale):
    """n transforms: a small turn about z, and z translations that differ from the neighbouring pair's by at least `step` (a
    turn about z leaves that difference in the moved point whatever the angles are)."""
    step = 0.1 * max(1.0, scale / 80.0)
    ang = rng.uniform(-0.05, 0.05, n)
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    T[:, 0, 3] = rng.uniform(-1, 1, n)
    T[:, 1, 3] = rng.uniform(-1, 1, n)
    T[:, 2, 3] = step * (np.arange(n) % 5 - 2)
    return T.astype(F)


def _pose(rng):
    a = 0.3
    pose = np.eye(4)
    pose[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]])
    pose[:3, 3] = (1.3, -0.2, 0.05)
    return pose.astype(F)


@pytest.mark.parametrize("scale", [1.0, 80.0, 3000.0])
def test_flow_rigid_rows_within_the_rounding_bound(scale):
    """The kernel rounds nine times per flow component: four forming a row of M = T pose (one product, three fmaf), four
    applying it to (x, y, z, 1), one subtracting the point.  Each of the first eight is relative to a partial sum bounded by
    (|T| |pose| p~)_r with p~ = (|x|, |y|, |z|, 1), the last to |moved_r - p_r| <= (|T| |pose| p~)_r + |p_r|; with u = 2^-24 and
    (1 + u)^9 - 1 < 10 u:   |got - exact| <= 10 u ((|T| |pose| p~)_r + |p_r|),   exact = the fp64 evaluation of the same float32
    inputs.  A lookup that is off by one pair misses this bound by at least 100 x (asserted on the inputs)."""
    rng = np.random.default_rng(int(scale))
    pose = _pose(rng)
    worst = 0.0
    for P in (0, 1, 2047, 2048, 2049, 4097):
        pair_labels = rng.permutation(P + 50)[:P].astype(F)
        if P >= 2:
            pair_labels[0] = pair_labels[P - 1]                       # a source label listed twice: the last one wins
        if P > 2049:
            pair_labels[5] = pair_labels[2050]                        # ... and twice in different label tiles
        T = _rigid(rng, max(P, 1), scale)[:P]
        rows10 = rng.normal(0, 1, (P, 10)).astype(F)
        rows10[:, 0] = pair_labels
        for N in (1, 255, 256, 257, 5000):
            labels = rng.integers(-1, P + 50, N).astype(F)
            if P:
                labels[::3] = pair_labels[rng.integers(0, P, len(labels[::3]))]
                labels[-1] = pair_labels[P - 1]
            pts = (rng.uniform(-1, 1, (N, 3)) * scale).astype(F)
            idx = lookup(labels, pair_labels)
            exact, mag = exact_flow(pts, idx, T, pose)
            bound = 10 * U * mag
            if P >= 3:
                aside = np.minimum(np.abs(exact_flow(pts, idx, T, pose, shift=1)[0] - exact).max(1),
                                   np.abs(exact_flow(pts, idx, T, pose, shift=-1)[0] - exact).max(1))
                inner = (idx > 0) & (idx < P - 1)                     # both neighbours exist
                assert (inner.any() or N == 1) and (aside[inner] >= 100 * bound[inner].max(1)).all(), (P, N)
            got = None
            for stride, rows in ((1, pair_labels), (10, rows10)):
                again = gpu_flow(pts, labels, rows, stride, T.reshape(P, 16), P, pose)
                assert got is None or np.array_equal(bits(got), bits(again))
                got = again
            ratio = np.abs(got.astype(np.float64) - exact) / bound
            worst = max(worst, float(ratio.max()))
            assert (ratio <= 1.0).all(), (P, N, float(ratio.max()))
    print(f"scale {scale:g} m: max |got - exact| / bound = {worst:.3f}")


def test_flow_on_the_padded_rows_of_collect():
    """The chain production runs: icpflow_flow_rigid_rows on collect's padded [cap,10] rows (stride 10, P = cap) is bit-identical
    to the flow from rows[:count] alone, for points that carry every matched label, unmatched labels, -1, -1e8, NaN and +-0.0
    against the matched label 0.0."""
    rng = np.random.default_rng(8)
    S, D = 6, 7
    src = np.array([0.0, 1.0, 2.0, 5.0, 7.0, 9.0])
    dst = np.arange(D, dtype=np.float64) + 20
    st1 = ar.plain_stage(S, D, [0, 2, 3], [1, 0, 6])
    st2 = ar.plain_stage(S, D, [4, 5], [2, 3], err=0.3)               # row 5 -> 3 only; err 0.3 is not below thres_error
    f1, f2 = ar.unpack(st1.result, 3), ar.unpack(st2.result, 2)
    f1.T[:] = _rigid(rng, 3, 80.0).reshape(3, 16)
    f2.T[:] = _rigid(rng, 2, 80.0).reshape(2, 16)
    f2.errors[0] = F(0.1)
    best1, best2 = gpu_assign(st1), gpu_assign(st2)
    assert np.array_equal(best1, [0, -1, 1, 2, -1, -1]) and np.array_equal(best2, [-1, -1, -1, -1, 0, -1])
    cap = 2 * S
    rows, T, count = gpu_collect(best1, st1, best2, st2, src[:, None], dst[:, None], 1, S, cap)
    assert count == 4 and np.array_equal(rows[:4, 0], [0.0, 2.0, 5.0, 7.0]) and (rows[4:, 0] == ar.FILL_LABEL).all()
    labels = np.array([0.0, -0.0, 2.0, 5.0, 7.0, 1.0, 9.0, 3.0, -1.0, -1e8, np.nan, 20.0, 26.0] * 41, F)
    pts = (rng.uniform(-1, 1, (len(labels), 3)) * 80).astype(F)
    pose = _pose(rng)
    padded = gpu_flow(pts, labels, rows, 10, T, cap, pose)
    alone = gpu_flow(pts, labels, rows[:count], 10, T[:count], count, pose)
    assert np.array_equal(bits(padded), bits(alone))
    idx = lookup(labels, rows[:count, 0])
    exact, mag = exact_flow(pts, idx, T[:count], pose)
    assert (idx >= 0).sum() == 5 * 41                                     # 0.0, -0.0, 2, 5, 7
    assert (np.abs(padded.astype(np.float64) - exact) <= 10 * U * mag).all()


# ------------------------------------------------------------------------------------------------ icpflow_gather_segments
def _gather_case(rng, B, N, M, subsample):
    """seg int64 [3,B], perm, and the expected rows per (pair, slot) as rows of the point table (-1: pad)."""
    seg = np.zeros((3, B), np.int64)
    perm, want = [], np.full((B, N), -1, np.int64)
    order = rng.permutation(M).astype(np.int64)
    for b in range(B):
        count = (0, 1, N - 1, N)[b % 4] if b < 4 or rng.random() < 0.5 else int(rng.integers(0, N + 1))
        if B == 1:
            count = N
        elif b == B - 1 and b >= 4:
            count = max(count, min(N, 3))                             # (the pair at the end of `order` takes rows)
        length = count + (int(rng.integers(1, 40)) if subsample and b % 2 == 1 else 0)    # an over-long cluster, subsampled
        start = M - length if b == B - 1 else int(rng.integers(0, M - length + 1))        # the last rows of `order`
        off = -1
        if length > count:
            off = len(perm)
            perm += list(rng.permutation(length)[:count])
            want[b, :count] = order[start + np.asarray(perm[off:off + count], np.int64)]
        else:
            want[b, :count] = order[start:start + count]
        seg[:, b] = (start, count, off)
    return order, seg, (np.asarray(perm, np.int32) if perm else None), want


@pytest.mark.parametrize("B,N", [(1, 1), (3, 85), (1, 255), (1, 256), (1, 257), (5, 1000), (4, 1), (8, 33)])
def test_gather_segments_equals_numpy_indexing(B, N):
    rng = np.random.default_rng(B * 1000 + N)
    M = 3000
    points = rng.uniform(-80, 80, (M, 3)).astype(F)
    for subsample in (False, True):
        for count_of_single in ((0, 1, N - 1, N) if B == 1 else (None,)):
            order, seg, perm, want = _gather_case(rng, B, N, M, subsample)
            if count_of_single is not None:                           # B = 1: every count in turn
                seg[1, 0] = count_of_single
                want[0, count_of_single:] = -1
                if seg[2, 0] < 0:
                    seg[0, 0] = M - count_of_single
                    want[0, :count_of_single] = order[M - count_of_single:]
            expect = np.empty((B, N, 4), F)
            expect[...] = (1e8, 1e8, 1e8, 0.0)
            valid = want >= 0
            expect[valid, :3] = points[want[valid]]
            expect[valid, 3] = 1.0
            assert subsample or perm is None
            d = [dev(points), dev(order), dev(seg), dev(perm)]
            out = Out((B, N, 4), F)
            _lib.call("icpflow_gather_segments", *[_lib.ptr(x) for x in d], B, N, out.ptr, _lib.stream(DEV))
            assert np.array_equal(bits(out.read()), bits(expect)), (subsample, count_of_single)
            # icpflow_gather_pad on the equivalent row list, -1 for the holes: the same batch
            rows = dev(want.astype(np.int32))
            out2 = Out((B, N, 4), F)
            _lib.call("icpflow_gather_pad", _lib.ptr(d[0]), _lib.ptr(rows), B, N, out2.ptr, _lib.stream(DEV))
            assert np.array_equal(bits(out2.read()), bits(expect))


# ----------------------------------------------------------------------------------------------- icpflow_transform_points
@pytest.mark.parametrize("B", [1, 300])
def test_transform_points_within_the_rounding_bound(B):
    """transform_points_batch (utils_helper.py:76-87).  Four roundings per component (one product, two fmaf, the sum with t), each
    relative to a partial sum bounded by (|R| |p| + |t|)_r; (1 + u)^4 - 1 < 5 u:   |got - exact| <= 5 u (|R| |p| + |t|)_r.  The w
    column is copied bit for bit, on pad rows too; in place gives the same bits."""
    rng = np.random.default_rng(B)
    worst = 0.0
    for N in (1, 255, 256, 257):
        xyz = np.empty((B, N, 4), F)
        xyz[:, :, :3] = rng.uniform(-80, 80, (B, N, 3))
        xyz[:, :, 3] = rng.integers(0, 1 << 32, (B, N), dtype=np.uint64).astype(np.uint32).view(F)     # any bits in w
        pad = rng.random((B, N)) < 0.2
        xyz[pad] = (1e8, 1e8, 1e8, 0.0)
        pose = np.stack([_rigid(rng, 1, 80.0)[0].astype(np.float64) @ _pose(rng).astype(np.float64) for _ in range(B)]).astype(F)
        x, p = dev(xyz), dev(pose)
        out = Out((B, N, 4), F)
        _lib.call("icpflow_transform_points", _lib.ptr(x), _lib.ptr(p), B, N, out.ptr, _lib.stream(DEV))
        got = out.read()
        R, t, pt = pose[:, :3, :3].astype(np.float64), pose[:, :3, 3].astype(np.float64), xyz[:, :, :3].astype(np.float64)
        exact = np.einsum("bij,bnj->bni", R, pt) + t[:, None, :]
        bound = 5 * U * (np.einsum("bij,bnj->bni", np.abs(R), np.abs(pt)) + np.abs(t)[:, None, :])
        ratio = np.abs(got[:, :, :3].astype(np.float64) - exact) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (N, float(ratio.max()))
        assert np.array_equal(bits(got[:, :, 3]), bits(xyz[:, :, 3]))
        inplace = Out((B, N, 4), F, fill=xyz)
        _lib.call("icpflow_transform_points", inplace.ptr, _lib.ptr(p), B, N, inplace.ptr, _lib.stream(DEV))
        assert np.array_equal(bits(inplace.read()), bits(got))
    print(f"B = {B}: max |got - exact| / bound = {worst:.3f}")

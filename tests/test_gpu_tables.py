"""The cluster tables on their own: what table_dict_kernel, table_count_kernel, table_scan_kernel, table_scatter_kernel and
table_stats_kernel (csrc/table.hip) leave behind icpflow_cluster_table / icpflow_cluster_table_pair, and cluster_stats_kernel
(csrc/pose.hip) behind icpflow_cluster_stats, against tests/table_restatement.py -- exactly: the number of labels, the WHOLE row
order (a stable sort: comparing it whole checks stability) and columns 0 - 2 of the rows; only the centroid gets a bound, derived
in table_restatement.centroid_bound and checked against exact rationals on the CPU (tests/test_table_restatement.py).

Every call is a raw C-ABI call with Lmax passed explicitly, on an exactly sized workspace filled with 0xFF, with guards round the
workspace, d_order, d_table and d_num (tests/table_device.py); rows of d_table from num on keep their poison.  Inputs:
tests/table_cases.py; that they hold the label counts, chunk counts, 64-label rounds and home slots their names claim is asserted
on the CPU.

Which input reaches what (read from csrc/table.hip):
  found <= 1024 / > 1024     the rank path / the bitonic network with its padding up to a power of two (label counts 1025 .. 4095)
  n > 1024 in the scan       rounds of 1024 labels joined by the carry (label counts 1025 .. 4096, read through order and starts)
  chunks 15, 16, 17, 32, 33  the 16-wide clamped load groups of the scan (M = 7680 .. 16385)
  home slots >= 8188         long probe chains and the wrap of the linear probe; one home slot for 1024 / 1025 labels
  rowOf above 511            every case with more than 512 labels
  rows 256 / 512 of a chunk  the two rows of a counting thread and its shortcut between them; M and label boundaries on these seams
  64 labels per round        64 ballot turns in every scatter round
  Measured figures (the largest share of the centroid bound, the time of the 20 000-label overflow) are printed, not gated.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

import table_cases as tc          # noqa: E402
import table_device as td         # noqa: E402
import table_restatement as tr    # noqa: E402

F = np.float32
POISON64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def check(res, labels, Lmax, what):
    """one table call against the restatement -> (order, rows) of the restatement, or None for an overflow"""
    order, rows, lab_bits = tr.table(labels)
    L = len(rows)
    if L > Lmax:
        # exact up to kDictMax + 1 = 4097 labels: table_dict_kernel's probes give up only once nFound > 4096, i.e. once all 4097 keys
        # are stored; beyond that the count is a lower bound
        assert res.num == -L if L <= 4097 else res.num < -4096, f"{what}: num = {res.num} for {L} labels at Lmax = {Lmax}"
        return None
    assert res.num == L, f"{what}: num = {res.num}, {L} labels"
    bad = np.flatnonzero(res.order != order)
    assert len(bad) == 0, f"{what}: order differs at {len(bad)} positions, the first {bad[:5]}: got {res.order[bad[:5]]}, want {order[bad[:5]]}"
    got = res.table[:L]
    assert np.array_equal(got[:, 0].astype(F).view(np.uint32), tr.quiet(lab_bits)), f"{what}: labels"
    quiet64 = np.where(np.isnan(got[:, 0]), np.uint64(1 << 51), np.uint64(0))      # (a conversion quiets a signalling NaN)
    assert np.array_equal(got[:, 0].astype(F).astype(np.float64).view(np.uint64) | quiet64, got[:, 0].view(np.uint64) | quiet64), f"{what}: a label that is no float32"
    assert np.array_equal(got[:, 1:3], rows[:, 1:3]), f"{what}: counts / starts differ in rows {np.flatnonzero((got[:, 1:3] != rows[:, 1:3]).any(axis=1))[:5]}"
    assert (res.table_words[L:] == POISON64).all(), f"{what}: rows from num on were written"
    return order, rows


def run(labels, Lmax, what, points=None, stream=None):
    res = td.table(tc.points_for(labels) if points is None else points, labels, Lmax, stream)
    return res, check(res, labels, Lmax, what)


@pytest.mark.parametrize("M", tc.SEAM_M)
def test_row_seams(M):
    """M on every seam of the chain: the wave of the scatter (64), the two rows of a counting thread (256), a chunk (512), the
    dictionary's round (8192), and 1 to 33 chunks -- 15, 16, 17, 32 and 33 among them, the 16-wide load groups of the scan."""
    for name, lab in tc.seam_patterns(M).items():
        run(lab, tc.LMAX, f"M = {M}, {name}")


@pytest.mark.parametrize("L", tc.LABEL_COUNTS)
def test_label_counts(L):
    """L distinct labels of alternating sign, 1 - 4 rows each, shuffled: the rank path up to 1024, the bitonic network beyond (L no
    power of two: its padding), the scan's rounds of 1024 labels.  Lmax = L gives what Lmax = 4096 gives (the stride of `counts`)."""
    lab = tc.counted(L)
    pts = tc.points_for(lab)
    wide, _ = run(lab, tc.LMAX, f"{L} labels at Lmax = 4096", pts)
    tight, _ = run(lab, L, f"{L} labels at Lmax = {L}", pts)
    assert np.array_equal(wide.order, tight.order) and np.array_equal(wide.table_words[:L], tight.table_words[:L])


@pytest.mark.parametrize("Lmax", [1, 7, 512, 4096])
def test_one_small_cloud_at_every_table_size(Lmax):
    lab = tc.small_cloud()
    _, w = run(lab, Lmax, f"five labels at Lmax = {Lmax}")
    assert (w is None) == (Lmax == 1)


@pytest.mark.parametrize("L,Lmax", tc.OVERFLOWS)
def test_overflow_reports_the_count(L, Lmax):
    _, w = run(tc.overflow(L), Lmax, f"{L} labels at Lmax = {Lmax}")
    assert w is None


def test_overflow_beyond_the_dictionary():
    """20 000 rows, 20 000 labels: num < -4096, no more is promised.  The time of the call is printed, not gated."""
    lab = tc.all_different()
    res, w = run(lab, tc.LMAX, "20 000 labels")
    assert w is None and res.num < -4096
    print(f"20 000 distinct labels at Lmax = 4096: num = {res.num}, the call took {res.seconds * 1e3:.3f} ms (enqueue to completion)")


def test_label_values():
    """-inf .. +inf in float order, denormals of both signs, 1.0 and its successor, 2^24; +-0.0 one cluster reported as 0.0 with its
    rows in original order."""
    lab, asc = tc.values()
    res, (order, rows) = run(lab, tc.LMAX, "label values")
    assert np.array_equal(res.table[:len(asc), 0].astype(F).view(np.uint32), asc.view(np.uint32))
    zero = int(np.flatnonzero(asc == 0)[0])
    rows_of_zero = res.order[int(rows[zero, 2]):int(rows[zero, 2] + rows[zero, 1])]
    assert np.array_equal(rows_of_zero, np.flatnonzero(lab == 0)) and len(rows_of_zero) == 7
    res, _ = run(tc.zeros_only(), 7, "both zeros")
    assert res.num == 3 and np.array_equal(res.order, [5, 0, 1, 3, 4, 2])
    assert np.array_equal(res.table[:3, :3].view(np.uint64), np.array([[-1, 1, 0], [0, 4, 1], [1, 1, 5]], np.float64).view(np.uint64))


def test_both_zeros_give_the_table_of_the_fallback():
    """The device table and ClusterTable._from_torch (the chain of torch ops behind an overflow) agree on a cloud with both zeros."""
    from icp_flow_amd.utils_check import ClusterTable
    rng = np.random.default_rng(17)
    lab = np.array([0.0, -0.0, 1.0, -1.0, 2.0], F)[rng.integers(0, 5, 700)]
    pts = tc.points_for(lab)
    dev = ClusterTable(td.G(pts), td.G(lab))
    ref = ClusterTable(td.G(pts), td.G(lab), fetch=False, _launch=False)
    ref._from_torch()
    assert len(dev.h_labels) == 4 and np.array_equal(dev.h_labels, ref.h_labels) and not np.signbit(dev.h_labels[1])
    assert torch.equal(dev.order, ref.order)
    for k in ("h_count", "h_start", "h_mean", "h_extent"):
        assert np.array_equal(getattr(dev, k), getattr(ref, k)), k
    assert int(dev.find(td.G(np.array([-0.0], F)))[0]) == 1 and dev.find_host(np.array([0.0], F))[0] == 1


def test_nan_labels():
    """The library's own rule (torch gives every NaN row a cluster of its own): one cluster per bit pattern, negative NaNs before
    -inf, positive NaNs after +inf, the NaN of all ones with its neighbour; statistics for all of them (NaN < 0 is false).  A
    signalling NaN of each sign keeps a cluster of its own beside its quiet form (label_key selects, it does not add), and reads back
    from the float64 column as that quiet form."""
    lab, want = tc.nans()
    pts = tc.points_for(lab)
    res, (order, rows) = run(lab, 64, "NaN labels", pts)
    assert res.num == len(want) == 14
    assert np.array_equal(res.table[:len(want), 0].astype(F).view(np.uint32), tr.quiet(want))
    mean, ext, mabs = tr.stats(pts, order, rows[:, 2], rows[:, 1], np.nan_to_num(rows[:, 0], nan=1.0))
    check_stats(res.table[:len(want), 3:6], res.table[:len(want), 6:9], mean, ext, mabs, rows[:, 1], "NaN labels")
    assert (res.table[:len(want)][np.isnan(rows[:, 0]), 6:9] > 0).any(axis=1).all()


@pytest.mark.parametrize("name", ["slot 8191", "slots 8188+", "slot 8191 in 3000", "slots 8188+ in 3000", "dense 1024", "dense 1025"])
def test_hash_chains(name):
    """Labels that all start in slot 8191 (at least 105 of 106 are stored past the wrap) or in the last four slots, alone (the rank
    path) and among 3000 others (the sorting network); 1024 and 1025 labels of ONE home slot, whose chain crosses the wrap."""
    lab = {"slot 8191": lambda: tc.hash_cloud(tc.hash_labels(8191)), "slots 8188+": lambda: tc.hash_cloud(tc.hash_labels(8188)),
           "slot 8191 in 3000": lambda: tc.hash_cloud(tc.hash_labels(8191), 3000), "slots 8188+ in 3000": lambda: tc.hash_cloud(tc.hash_labels(8188), 3000),
           "dense 1024": lambda: tc.hash_cloud(tc.dense_labels(1024)), "dense 1025": lambda: tc.hash_cloud(tc.dense_labels(1025))}[name]()
    _, w = run(lab, tc.LMAX, name)
    assert w is not None


@pytest.mark.parametrize("name", ["round of 64", "giant", "once per chunk"])
def test_contention_and_stability(name):
    """64 different labels in every scatter round (64 ballot turns, each group in an order of its own); one label on 70 % of 20 000
    rows beside 500 singletons; 300 labels exactly once per chunk (every count of a chunk is 1: the running offsets carry the order)."""
    lab = {"round of 64": tc.round_of_64, "giant": tc.giant, "once per chunk": tc.once_per_chunk}[name]()
    _, w = run(lab, tc.LMAX, name)
    assert w is not None


@pytest.mark.parametrize("name", list(tc.pair_cases()))
def test_pair_form(name):
    """icpflow_cluster_table_pair: every output bit for bit that of two single calls and equal to the restatement; a side that
    overflows leaves the other side whole."""
    la, lb, Lmax = tc.pair_cases()[name]
    pa, pb = tc.points_for(la, 1), tc.points_for(lb, 2)
    ra, rb = td.table_pair(pa, la, pb, lb, Lmax)
    for res, pts, lab, side in ((ra, pa, la, "A"), (rb, pb, lb, "B")):
        w = check(res, lab, Lmax, f"pair {name}, side {side}")
        one = td.table(pts, lab, Lmax)
        assert res.num == one.num, side
        if w is not None:
            assert np.array_equal(res.order_words, one.order_words), side
            assert np.array_equal(res.table_words, one.table_words), side     # (statistics and the poison behind num included)


def check_stats(got_mean, got_ext, mean, ext, mabs, count, what):
    assert np.array_equal(got_mean.astype(F).astype(np.float64).view(np.uint64), got_mean.view(np.uint64)), f"{what}: a centroid that is no float32"
    assert np.array_equal(np.asarray(got_ext, np.float64), ext.astype(np.float64)), f"{what}: extents differ in clusters {np.flatnonzero((got_ext != ext).any(axis=1))[:5]}"
    bound = tr.centroid_bound(mean, np.asarray(count)[:, None], mabs)
    err = np.abs(np.asarray(got_mean, np.float64) - mean)
    share = float((err / bound).max())
    assert (err <= bound).all(), f"{what}: centroid off by {share:.3f} of the bound in cluster {int(np.argmax((err / bound).max(axis=1)))}"
    return share, float((err / bound)[np.asarray(count) > 2].max(initial=0.0))


@pytest.mark.parametrize("name", list(tc.stat_cases()))
def test_statistics(name):
    """Clusters of 1 .. 70 000 rows (the four rows of a thread and round of table_stats_kernel: 1023 .. 1025, 4095 .. 4097, 8193)
    at the origin, at (3000, -7000, 30) and at +-1e6 m, where a float32 step is 1 / 16 m; boxes in all six axis orders, with two
    and with three equal extents; 1 and 4096 clusters.  Extents exactly numpy's float32 result; the centroid within the derived
    bound of fsum / n; through the table and through icpflow_cluster_stats with d_labels given and NULL (negative labels then get
    statistics), the two kernels bit for bit the same."""
    pts, lab = tc.stat_cases()[name]
    res, (order, rows) = run(lab, tc.LMAX, f"statistics, {name}", pts)
    L = len(rows)
    labels, count, start = rows[:, 0].astype(F), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64)
    mean, ext, mabs = tr.stats(pts, order, start, count, labels)
    share, share3 = check_stats(res.table[:L, 3:6], res.table[:L, 6:9], mean, ext, mabs, count, f"{name}, table_stats_kernel")
    assert (res.table[:L][labels < 0, 3:9] == 0).all()
    m1, e1 = td.cluster_stats(pts, order, start, count, labels)
    assert np.array_equal(m1.astype(np.float64).view(np.uint64), res.table[:L, 3:6].view(np.uint64)), "the two statistics kernels differ (centroid)"
    assert np.array_equal(e1.astype(np.float64).view(np.uint64), res.table[:L, 6:9].view(np.uint64)), "the two statistics kernels differ (extents)"
    m0, e0 = td.cluster_stats(pts, order, start, count, None)
    mean0, ext0, mabs0 = tr.stats(pts, order, start, count, None)
    check_stats(m0.astype(np.float64), e0, mean0, ext0, mabs0, count, f"{name}, cluster_stats_kernel without labels")
    keep = ~(labels < 0)
    assert np.array_equal(m0[keep].view(np.uint32), m1[keep].view(np.uint32)) and np.array_equal(e0[keep].view(np.uint32), e1[keep].view(np.uint32))
    # (a cluster of two rows one float32 step apart has its mean on a tie: a share of exactly 1; clusters of more than two rows apart)
    print(f"{name}: largest share of the centroid bound {share:.3f} (clusters of more than two rows: {share3:.3f})")


def test_reruns_and_a_second_stream_leave_the_same_bits():
    """Four runs on two streams: num, the whole order and the rows (statistics included) the same bits."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64))      # noqa: E731
    side = torch.cuda.Stream()
    for pts, lab in (tc.stat_cloud("3 km"), (None, tc.counted(3000)), (None, tc.giant())):
        pts = tc.points_for(lab) if pts is None else pts
        runs = [td.table(pts, lab, tc.LMAX, s) for s in (None, side, None, side)]
        check(runs[0], lab, tc.LMAX, "first run")
        for r in runs[1:]:
            assert r.num == runs[0].num and torch.equal(T(r.order_words), T(runs[0].order_words)) and torch.equal(T(r.table_words), T(runs[0].table_words))

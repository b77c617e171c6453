"""CPU-only: tests/table_restatement.py against two independent statements of the same table (numpy's unique and stable argsort of
the float values; the torch ops the chain of launches replaced), the conditions every input of tests/table_cases.py was built for
-- conditions on the inputs, not measurements of the kernels -- and the centroid bound of the GPU test against exact rationals."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import table_cases as tc          # noqa: E402
import table_restatement as tr    # noqa: E402

F = np.float32


def every_label_case():
    """-> {name: labels}: every labelled cloud of the GPU test that holds no NaN"""
    out = {}
    for M in tc.SEAM_M:
        for name, lab in tc.seam_patterns(M).items():
            out[f"seam {M} {name}"] = lab
    for L in tc.LABEL_COUNTS:
        out[f"counted {L}"] = tc.counted(L)
    for L, _ in tc.OVERFLOWS:
        out[f"overflow {L}"] = tc.overflow(L)
    out.update({"small": tc.small_cloud(), "all different": tc.all_different(), "values": tc.values()[0], "zeros": tc.zeros_only(),
                "slot 8191": tc.hash_cloud(tc.hash_labels(8191)), "slots 8188+": tc.hash_cloud(tc.hash_labels(8188)),
                "slot 8191 in 3000": tc.hash_cloud(tc.hash_labels(8191), 3000), "slots 8188+ in 3000": tc.hash_cloud(tc.hash_labels(8188), 3000),
                "dense 1024": tc.hash_cloud(tc.dense_labels(1024)), "dense 1025": tc.hash_cloud(tc.dense_labels(1025)),
                "round of 64": tc.round_of_64(), "giant": tc.giant(), "once per chunk": tc.once_per_chunk(),
                "denormals": np.array([1e-45, -1e-45, 0.0, 1e-40, -0.0, 1e-45, -1e-40, 1e-38], F)})
    for name, (la, lb, _) in tc.pair_cases().items():
        out[f"pair {name} A"], out[f"pair {name} B"] = la, lb
    for name, (_, lab) in tc.stat_cases().items():
        out[f"stat {name}"] = lab
    return out


CASES = every_label_case()


def test_the_restatement_equals_numpy_and_the_torch_ops_on_every_case():
    """np.unique with counts and a stable argsort of the FLOAT values; torch argsort(stable) / unique_consecutive / cumsum: the same
    order, labels (as values: both zeros equal), counts and starts -- on every case, +-0.0, +-inf and denormals included."""
    for name, lab in CASES.items():
        assert not np.isnan(lab).any(), name
        order, rows, lab_bits = tr.table(lab)
        uniq, count = np.unique(lab, return_counts=True)
        assert np.array_equal(order, np.argsort(lab, kind="stable")), name
        assert np.array_equal(rows[:, 0], uniq.astype(np.float64)) and np.array_equal(rows[:, 1], count), name
        assert np.array_equal(rows[:, 2], np.cumsum(count) - count), name
        assert not (lab_bits == 0x80000000).any(), f"{name}: a zero label is reported as -0.0"
        t = torch.from_numpy(lab)
        o = torch.argsort(t, stable=True)
        u, c = torch.unique_consecutive(t[o], return_counts=True)
        assert np.array_equal(order, o.numpy()), name
        assert np.array_equal(rows[:, 0], u.double().numpy()) and np.array_equal(rows[:, 1], c.numpy()), name
        assert np.array_equal(rows[:, 2], (torch.cumsum(c, 0) - c).numpy()), name


def test_keys_keep_the_float_order_and_come_back():
    rng = np.random.default_rng(0)
    f = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(F)
    f = np.concatenate([f[~np.isnan(f)], tc.values()[1]])
    k = tr.key(f)
    o = np.argsort(k, kind="stable")
    assert (np.diff(f[o].astype(np.float64)) >= 0).all()
    assert np.array_equal((np.diff(k[o].astype(np.int64)) == 0), (np.diff(f[o].astype(np.float64)) == 0))      # equal keys: equal values
    assert np.array_equal(tr.label_of(k), np.where(f == 0, F(0.0), f)) and not (tr.bits(tr.label_of(k)) == 0x80000000).any()
    assert tr.key(np.array([-0.0], F))[0] == tr.key(np.array([0.0], F))[0] == 0x80000000
    assert (k != tr.EMPTY).all() and tr.key(np.array([0x7FFFFFFF], np.uint32).view(F))[0] == tr.EMPTY - 1


def test_the_nan_rule_of_the_restatement():
    lab, want = tc.nans()
    order, rows, lab_bits = tr.table(lab)
    assert np.array_equal(lab_bits, want)
    assert np.array_equal(tr.bits(lab)[order[int(rows[-1, 2]):]] | 1, np.full(int(rows[-1, 1]), 0x7FFFFFFF, np.uint32))   # all ones and its neighbour: one cluster
    assert np.isneginf(rows[5, 0]) and np.isposinf(rows[8, 0]) and np.isnan(rows[:5, 0]).all() and np.isnan(rows[9:, 0]).all()
    # a signalling NaN of each sign is among them, a cluster of its own next to its quiet form, which it reads back as
    assert lab_bits[4] == 0xFF800001 and lab_bits[9] == 0x7F800001 and {0xFFC00001, 0x7FC00001} <= set(lab_bits.tolist())
    assert tr.quiet(lab_bits)[4] == 0xFFC00001 and tr.quiet(lab_bits)[9] == 0x7FC00001
    assert np.array_equal(tr.quiet(tr.bits(tc.values()[1])), tr.bits(tc.values()[1]))               # (no other pattern changes)
    assert (rows[np.isnan(rows[:, 0]), 1] >= 2).all()
    for c in range(len(rows)):                                               # rows of a cluster in original order
        assert (np.diff(order[int(rows[c, 2]):int(rows[c, 2] + rows[c, 1])]) > 0).all()


def test_inputs_hold_the_label_counts_they_were_built_for():
    n = lambda lab: len(tr.table(lab)[1])      # noqa: E731
    for M in tc.SEAM_M:
        p = tc.seam_patterns(M)
        assert all(len(lab) == M for lab in p.values())
        assert n(p["one label"]) == 1 and n(p["two alternating"]) == min(M, 2) and n(p["seven iid"]) <= 7 and n(p["runs of 256"]) <= 4
        assert M < 200 or n(p["seven iid"]) == 7
        assert M < 1000 or n(p["sorted runs"]) == 37
        assert (np.diff(p["sorted runs"]) >= 0).all()
        assert ("every row its own" in p) == (M <= tc.LMAX) and (M > tc.LMAX or n(p["every row its own"]) == M)
        # the boundaries of "runs of 256" fall on rows 256 and 512 of a chunk and nowhere else
        edge = np.flatnonzero(np.diff(p["runs of 256"]) != 0) + 1
        assert (edge % 256 == 0).all() and (M <= 1024 or set(edge % 512) == {0, 256})      # (0: the seam between two chunks)
    for L in tc.LABEL_COUNTS:
        order, rows, _ = tr.table(tc.counted(L))
        assert len(rows) == L and rows[:, 1].min() >= 1 and rows[:, 1].max() <= 4 and (L < 63 or rows[:, 1].max() == 4)
        assert L < 3 or ((rows[:, 0] < 0).any() and (rows[:, 0] > 0).any())
        first_seen = tc.counted(L)[np.sort(np.unique(tc.counted(L), return_index=True)[1])]
        assert L < 63 or (np.diff(first_seen) < 0).any()                    # the ascending order is not the order of arrival
    for L, Lmax in tc.OVERFLOWS:
        assert n(tc.overflow(L)) == L == Lmax + 1
    assert n(tc.small_cloud()) == 5 and n(tc.all_different()) == 20000 and len(tc.all_different()) == 20000
    lab, asc = tc.values()
    assert n(lab) == len(asc) == 13 and (np.diff(asc.astype(np.float64)) > 0).all()
    assert (tr.bits(lab) == 0x80000000).sum() == 3 and (tr.bits(lab) == 0).sum() == 4
    order, rows, _ = tr.table(tc.zeros_only())
    assert np.array_equal(order, [5, 0, 1, 3, 4, 2]) and np.array_equal(rows, [[-1, 1, 0], [0, 4, 1], [1, 1, 5]])
    assert n(tc.giant()) == 506 and (tc.giant() == 7.0).sum() == 14000 and (tr.table(tc.giant())[1][:, 1] == 1).sum() == 500
    assert n(tc.once_per_chunk()) == 301
    for name, (la, lb, Lmax) in tc.pair_cases().items():
        assert ("overflow x" in name) == (n(la) > Lmax) and ("x overflow" in name) == (n(lb) > Lmax), name
    assert n(tc.pair_cases()["1500 labels x 3"][0]) == 1500 and n(tc.pair_cases()["1500 labels x 3"][1]) == 3
    assert [(len(a), len(b)) for a, b, _ in list(tc.pair_cases().values())[:6]] == tc.PAIR_M


def test_seam_sizes_give_the_chunk_counts_they_were_built_for():
    assert [tr.chunks(M) for M in tc.SEAM_M] == tc.SEAM_CHUNKS
    assert {15, 16, 17, 32, 33} <= set(tc.SEAM_CHUNKS)                      # the 16-wide load groups of the scan: below, at, above, twice
    assert {tr.DICT_ROUND - 1, tr.DICT_ROUND, tr.DICT_ROUND + 1} <= set(tc.SEAM_M)
    assert {tr.CHUNK // 2 - 1, tr.CHUNK // 2, tr.CHUNK // 2 + 1, tr.CHUNK - 1, tr.CHUNK, tr.CHUNK + 1} <= set(tc.SEAM_M)
    assert tr.chunks(len(tc.stat_cloud("origin")[1])) > 33


def test_every_scatter_round_holds_64_different_labels():
    lab = tc.round_of_64()
    assert len(lab) == 4096
    groups = lab.reshape(-1, 64)
    assert all(len(np.unique(g)) == 64 for g in groups)
    assert len({g.tobytes() for g in groups}) == len(groups)               # an order of its own per group
    assert len(np.unique(lab)) == 64
    lab = tc.once_per_chunk()
    for c in range(tr.chunks(len(lab))):
        v, n = np.unique(lab[c * tr.CHUNK:(c + 1) * tr.CHUNK], return_counts=True)
        assert (n[v != -1] == 1).all() and (v != -1).sum() == 300


def test_hash_cases_start_where_they_were_built_to():
    """The slot function restated.  K keys with home slot 8191: at most one of them sits in slot 8191, so at least K - 1 are
    stored past the wrap whatever the order of insertion."""
    assert tr.home_slot(np.array([0x80000000], np.uint32))[0] == 4096      # (an odd multiplier keeps the top bit)
    assert tr.home_slot(np.array([0x80000001], np.uint32))[0] == ((0x80000001 * 2654435761) % (1 << 32)) >> 19
    for want in (11885, 14340, 17206):
        assert tr.home_slot(tr.key(np.array([want], F)))[0] == 8191
    last, tail = tc.hash_labels(8191), tc.hash_labels(8188)
    assert len(last) >= 100 and (tr.home_slot(tr.key(last)) == 8191).all() and len(np.unique(last)) == len(last)
    assert len(tail) >= 400 and (tr.home_slot(tr.key(tail)) >= 8188).all() and len(np.unique(tail)) == len(tail)
    assert len(last) == 106 and len(tail) == 498                           # (the counts the cases were sized by)
    for n in (1024, 1025):
        d = tc.dense_labels(n)
        assert len(d) == n == len(np.unique(d)) and (tr.home_slot(tr.key(d)) == tc.DENSE_HOME).all()
        assert tc.DENSE_HOME + n - 1 > tr.SLOTS - 1                           # one home slot: the chain runs over the wrap
    # mixed into 3000 other labels: past 1024 labels (the sorting network), the chain still whole
    lab = tc.hash_cloud(tail, 3000)
    assert len(tr.table(lab)[1]) == 3000 + 498 and np.isin(tail, lab).all()
    # the labels 0 .. 4095 never probe past two slots and never wrap: what the suite ran before these cases
    h = np.sort(tr.home_slot(tr.key(np.arange(4096, dtype=F))))
    assert h.max() < tr.SLOTS - 1 and np.bincount(h.astype(np.int64)).max() <= 2


def round_sum(x, how):
    x = np.asarray(x, np.float64)
    if how == "sequential":
        s = 0.0
        for v in x.tolist():
            s += v
        return s
    if how == "pairwise":
        return float(np.add.reduce(x))
    # the kernels' shape: 1024 running sums over the rows 1024 apart, then those added up
    lanes = np.zeros(1024)
    for i0 in range(0, len(x), 1024):
        part = x[i0:i0 + 1024]
        lanes[:len(part)] += part
    return round_sum(lanes[:min(len(x), 1024)], "sequential")      # (the other lanes hold zeros)


@pytest.mark.parametrize("name", list(tc.stat_cases()))
def test_the_centroid_bound_holds_for_an_fp64_sum_rounded_to_float32(name):
    """Exact rationals: for every cluster and axis of the statistics cases, float32(fp64 sum / n) in three orders of addition lies
    within tr.centroid_bound of the restatement's m = fsum / n -- so the GPU test's tolerance is a checked condition on its inputs
    -- and m within the bound's second term of the exact mean.  "Equals the nearest float32" is NOT claimed: the fp64 quotient can
    round to the neighbour of the exact mean's nearest float32."""
    pts, lab = tc.stat_cases()[name]
    order, rows, _ = tr.table(lab)
    mean, ext, mabs = tr.stats(pts, order, rows[:, 2], rows[:, 1], rows[:, 0])
    worst = Fraction(0)
    hows = ("sequential", "pairwise", "lanes")
    for c in range(len(rows)):
        n = int(rows[c, 1])
        if rows[c, 0] < 0:
            assert not mean[c].any() and not ext[c].any()
            continue
        x = pts[order[int(rows[c, 2]):int(rows[c, 2]) + n]].astype(np.float64)
        for a in range(3):
            exact = tr.exact_sum(x[:, a]) / n
            assert tr.exact_sum(np.abs(x[:, a])) / n <= Fraction(float(mabs[c, a])) * (1 + Fraction(1, 1 << 50))
            bound = Fraction(float(tr.centroid_bound(mean[c, a], n, mabs[c, a])))
            assert abs(Fraction(float(mean[c, a])) - exact) <= Fraction(2, 1 << 53) * Fraction(float(mabs[c, a])) * (1 + Fraction(1, 1 << 50))
            for how in hows:
                got = Fraction(float(F(round_sum(x[:, a], how) / n)))
                assert abs(got - Fraction(float(mean[c, a]))) <= bound, (name, c, a, how)
                worst = max(worst, abs(got - Fraction(float(mean[c, a]))) / bound)
    assert worst <= 1
    print(f"{name}: largest share of the centroid bound on the CPU {float(worst):.3f}")


def test_statistics_cases_hold_the_boxes_they_were_built_for():
    pts, lab = tc.stat_cloud("origin")
    order, rows, _ = tr.table(lab)
    assert [int(r[1]) for r in rows if r[0] >= 0] == tc.STAT_SIZES and (rows[:, 0] < 0).sum() == 2
    assert len(tc.stat_one_cluster()[1]) == 5000 and len(tr.table(tc.stat_many_clusters()[1])[1]) == 4096
    for name in tc.STAT_CENTRES:
        pts, lab = tc.stat_cloud(name)
        order, rows, _ = tr.table(lab)
        _, ext, _ = tr.stats(pts, order, rows[:, 2], rows[:, 1], rows[:, 0])
        for j, n in enumerate(tc.STAT_SIZES):
            c = int(np.flatnonzero(rows[:, 0] == j)[0])
            want = np.sort(np.array(tc.STAT_BOXES[j % len(tc.STAT_BOXES)], F)) if n >= 2 else np.zeros(3, F)
            assert np.array_equal(ext[c], want), (name, n)                  # the corners are float32 numbers: the extents exact
    # all six axis orders, the three places of an equal pair, three equal: each used by a cluster of at least two rows
    assert len(set(tc.STAT_BOXES)) == 10 and len([n for n in tc.STAT_SIZES if n >= 2]) >= 10

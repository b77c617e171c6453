"""A plain numpy restatement of icpflow_nn_residual_segments (include/icpflow_hip.h, 8(g)): the per-row search of
tests/residual_restatement.py once per side -- BEFORE: `before` as it is; AFTER: `after` + `flow` --, the segments by
tests/table_restatement.py's label rule (distinct labels ascending, -0.0 and +0.0 one label, NaN labels per bit pattern), and
per segment and side the good rows, the hits, the rows with d <= edge and the sums of d and d * d through math.fsum."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import residual_restatement as rr        # noqa: E402
import table_restatement as tr           # noqa: E402

COLS, SIDE, MAX_EDGES = 18, 8, 4
SKIP = (-1e8, -1.0)


def _side(d2, idx, members, edges):
    d = np.sqrt(np.asarray(d2, np.float32)).astype(np.float64)      # float32 square root, correctly rounded, then widened
    good = idx != -2
    L, E = len(members), len(edges)
    out = dict(rows=np.zeros(L, np.int64), hits=np.zeros(L, np.int64), under=np.zeros((L, E), np.int64), dsum=np.zeros(L), ddsum=np.zeros(L))
    for c, rows in enumerate(members):
        mine = rows[good[rows]]
        out["rows"][c] = len(mine)
        out["hits"][c] = int((idx[mine] >= 0).sum())
        for e, edge in enumerate(edges):
            out["under"][c, e] = int((d[mine] <= float(edge)).sum())
        out["dsum"][c] = math.fsum(d[mine].tolist())
        out["ddsum"][c] = math.fsum((d[mine] * d[mine]).tolist())
    return out


def residual(before, after, flow, labels, target, radius=2.0, edges=()):
    """-> dict(labels float64 [L], label_bits uint32 [L] (of the float32 label), rows int64 [L], before, after: dict(rows, hits,
    under, dsum, ddsum) per segment, d2_before, d2_after float32 [n], idx_before, idx_after int32 [n], info: the call's six
    words as far as the restatement knows them (bad queries before, after, bad targets))"""
    d2b, idxb, ib = rr.search(before, target, None, radius)
    d2a, idxa, ia = rr.search(after, target, flow, radius)
    order, rows, label_bits = tr.table(np.asarray(labels, np.float32).reshape(-1))
    members = [order[int(s): int(s) + int(c)] for _, c, s in rows]
    return dict(labels=rows[:, 0].copy() if len(rows) else np.zeros(0), label_bits=label_bits, rows=rows[:, 1].astype(np.int64) if len(rows) else np.zeros(0, np.int64),
                before=_side(d2b, idxb, members, edges), after=_side(d2a, idxa, members, edges), d2_before=d2b, d2_after=d2a,
                idx_before=idxb, idx_after=idxa, info=(ib["bad_queries"], ia["bad_queries"], ib["bad_targets"]))


def table18(res):
    """the restatement as the kernel's float64 [L][18]"""
    L = len(res["rows"])
    t = np.zeros((L, COLS))
    t[:, 0], t[:, 1] = res["labels"], res["rows"]
    for at, side in ((2, res["before"]), (2 + SIDE, res["after"])):
        E = side["under"].shape[1]
        t[:, at], t[:, at + 1], t[:, at + 2: at + 2 + E] = side["rows"], side["hits"], side["under"]
        t[:, at + 2 + MAX_EDGES], t[:, at + 3 + MAX_EDGES] = side["dsum"], side["ddsum"]
    return t


def means(side):
    """per segment the mean truncated distance (NaN without a good row)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return side["dsum"] / side["rows"]

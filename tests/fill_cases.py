"""The inputs the tests of the track fill share (tests/test_tracks_fill.py on the CPU, tests/test_gpu_tracks_fill.py on the GPU):
hand-made observation and segment tables for the plan, box tables for the candidates, seeded tables of both, and the end-to-end
scene (tests/repair_cases.scene, with one pair row deleted by the test).  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repair_cases as rc                     # noqa: E402

F = np.float32
S = 0.125                                      # seconds per sweep in the hand-made tables: binary fractions, exact sums
scene, displacement = rc.scene, rc.displacement
FRAMES, SWEEP_SECONDS, CLUSTER = rc.FRAMES, rc.SWEEP_SECONDS, rc.CLUSTER
FILLED, FILLED_FRAME = rc.FAULTED, rc.FAULTED_FRAME          # object 0's pair is deleted in gap 2: constant velocity, to be filled
HONEST, HONEST_FRAME = rc.HONEST, rc.HONEST_FRAME            # the box that truly leaves its line, its pair deleted where it left


def obs(track, gap, seconds, d, centre=(0.0, 0.0, 0.0), size=(4.0, 2.0, 1.5), points=50):
    """one observation row (icpflow_object_tracks_extend's columns): id, gap, seconds, d, size, points, the source box's centre"""
    return [track, gap, seconds, d[0], d[1], d[2], size[0], size[1], size[2], points, centre[0], centre[1], centre[2]]


def segment(label, rows, track, inherited=1.0):
    return [label, rows, track, inherited, 0.0, 1.0]


def on_a_line(seen=(1, 3), v=(2.0, -1.0, 0.25), land=(8.0, -4.0, 1.0), track=0, off=None):
    """a track seen once in every gap of `seen` at d = s v, every observation landing on `land` (c = land - d); off: {gap: offset
    added to that gap's d}"""
    rows = []
    for g in seen:
        d = np.array(v) * (S * g) + np.array((off or {}).get(g, (0.0, 0.0, 0.0)))
        rows.append(obs(track, g, S * g, d, np.array(land) - d))
    return rows


def slots(gaps=(1, 2, 3), segments=None, Lmax=4):
    """the segment tables of the slots of `gaps`: in every slot segment 0 is noise (no id), segment 1 carries track 0 (label 5,
    40 rows) unless `segments` says otherwise -> (segments [G, Lmax, 6], num [G], gaps, seconds)"""
    G = len(gaps)
    seg = np.zeros((G, Lmax, 6))
    num = np.zeros(G, np.int32)
    for g in range(G):
        rows = [segment(-1.0, 7, -1, 0.0), segment(5.0, 40, 0)] if segments is None else segments[g]
        seg[g, : len(rows)] = rows
        num[g] = len(rows)
    return seg, num, np.array(gaps, np.int32), np.array([S * g for g in gaps])


def random_plans(count=300, seed=23):
    """seeded inputs of the plan: ids -1, ids >= T, gaps outside [0, 63] among the observations, several rows of a track in one
    gap, slots whose tracks are observed, unobserved, seen once, off their line; a negative count in a slot now and then"""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 3, 5, 63])
    for _ in range(count):
        M, T, Lmax = int(rng.integers(0, 30)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
        G = int(rng.integers(1, 5))
        gaps = rng.choice(pool, G, replace=False)
        v = rng.normal(0, 3, (T + 3, 3))
        rows = []
        for _ in range(M):
            t = int(rng.integers(-1, T + 2))
            g = int(rng.choice([-1, 0, 1, 2, 3, 5, 63, 64, 70]))
            s = 0.1 * max(g, 1)
            d = s * v[t + 1] + rng.normal(0, 0.15, 3) * (rng.random() < 0.3)
            rows.append(obs(t, g, s, d, rng.normal(0, 20, 3)))
        seg = rng.normal(0, 1, (G, Lmax, 6))
        seg[:, :, 2] = rng.integers(-1, T + 2, (G, Lmax))
        seg[:, :, 0], seg[:, :, 1] = rng.integers(0, 50, (G, Lmax)), rng.integers(1, 500, (G, Lmax))
        num = rng.integers(0, Lmax + 1, G).astype(np.int32)
        if rng.random() < 0.1:
            num[int(rng.integers(0, G))] = -int(rng.integers(1, 9))
        yield dict(obs=np.array(rows).reshape(M, 13), T=T, segments=seg, num=num, gaps=gaps.astype(np.int32), seconds=0.1 * np.maximum(gaps, 1))


def plan_at(M, G, num, Lmax, seed):
    """a plan input at given sizes: a handful of tracks on their lines over the slots' gaps, a few observations off"""
    rng = np.random.default_rng(seed)
    gaps = np.arange(G, dtype=np.int32) if G > 3 else np.arange(1, G + 1, dtype=np.int32)
    T = max(2, min(40, M // 3))
    v = rng.normal(0, 3, (T, 3))
    land = rng.normal(0, 30, (T, 3))
    rows = []
    for _ in range(M):
        t = int(rng.integers(-1, T + 1))
        g = int(rng.choice([v for k, v in enumerate(gaps) if G == 1 or k != t % G]))      # track t has no pair in slot t mod G
        s = 0.1 * max(g, 1)
        d = s * v[t % T] + rng.normal(0, 0.3, 3) * (rng.random() < 0.1)
        rows.append(obs(t, g, s, d, land[t % T] - d))
    seg = np.zeros((G, Lmax, 6))
    seg[:, :, 0] = np.arange(Lmax)
    seg[:, :, 1] = rng.integers(1, 900, (G, Lmax))
    seg[:, :, 2] = rng.integers(-1, T + 1, (G, Lmax))
    return dict(obs=np.array(rows).reshape(M, 13), T=T, segments=seg, num=np.asarray(num, np.int32), gaps=gaps, seconds=0.1 * np.maximum(gaps, 1))


# -------------------------------------------------------------------------------------------------------------- the candidates

def box(label, centre, rows=50, k=0):
    """one row of icpflow_segment_boxes' table with what the candidates read: label, rows, k (-1: no box), the centre"""
    row = np.zeros(16)
    row[0], row[1], row[2], row[3], row[6:9] = label, rows, rows, k, centre
    return row


def box_table(rows, Lmax=None):
    table = np.zeros((Lmax or max(len(rows), 1), 16))
    if len(rows):
        table[: len(rows)] = rows
    return table


def pair_rows(labels, stride=10, seed=0):
    """pair rows whose column 0 holds `labels`, the other columns noise"""
    rows = np.random.default_rng(seed).random((len(labels), stride)).astype(F)
    rows[:, 0] = np.asarray(labels, F)
    return rows


def random_candidates(K, num, P, seed, Lmax=None, aimed=True):
    """seeded inputs of the candidates: boxes on a 3 m grid with a few without a box, too long, or matched; the rows aim near
    boxes (some beyond the radius, some at a matched one) and, with `aimed`, three of them at one segment"""
    rng = np.random.default_rng(seed)
    Lmax = Lmax or max(num, 1)
    rows = []
    for c in range(num):
        rows.append(box(float(c), (3.0 * (c % 64), 3.0 * (c // 64), 1.0), rows=int(rng.choice([50, 50, 50, 20000])), k=int(rng.choice([0, 3, 3, -1]))))
    table = box_table(rows, Lmax)
    table[num:] = rng.normal(0, 1, (Lmax - num, 16))                 # rows from the number on hold anything
    labels = rng.integers(0, max(num, 1) + 5, P).astype(F)
    q = np.zeros((K, 3))
    for k in range(K):
        c = int(rng.integers(0, max(num, 1)))
        q[k] = (3.0 * (c % 64) + rng.normal(0, 0.5), 3.0 * (c // 64) + rng.normal(0, 0.5), rng.normal())
    if aimed and K >= 3 and num >= 1:
        open_ = [c for c in range(num) if table[c, 3] >= 0 and table[c, 1] <= 10000 and float(c) not in set(labels.tolist())]
        if open_:
            c = open_[len(open_) // 2]
            q[:3] = table[c, 6:9] + np.array([[0.25, 0.0, 0.0], [0.0, 0.125, 5.0], [0.0, -0.125, 0.0]])   # rows 1 and 2 tie: the lower k keeps it
    return dict(q=q, boxes=table, num=num, pairs=pair_rows(labels, seed=seed))

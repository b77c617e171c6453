"""What the GPU tests of the track repair share, in the manner of tests/track_device.py: the raw calls of
icpflow_object_tracks_suspects, icpflow_pairs_repair_select and icpflow_pairs_reregister on buffers the test owns -- a workspace
of EXACTLY the size the library asks for, filled with 0xFF, between two guards, and every output between two guards in an
allocation of its own, poisoned beforehand -- and the comparison, np.array_equal (NaN = NaN) throughout, with
tests/repair_restatement.py.  Not a test module."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_device as bd                  # noqa: E402
import repair_restatement as rr          # noqa: E402
import residual_device as rd             # noqa: E402
import track_device as td                # noqa: E402

GUARD, DEV, upload = rd.GUARD, rd.DEV, rd.upload
F = np.float32
WS_POISON, POISON_WORD = bd.WS_POISON, bd.POISON_WORD
same, Buffers = bd.same, td.Buffers


def run_plan(obs, T, max_residual=0.2, stream=None):
    """One call of icpflow_object_tracks_suspects -> (plan [M, 8], counts [4], the outputs' bytes)"""
    from icp_flow_amd import _lib
    L = _lib._L
    obs = np.asarray(obs, np.float64).reshape(-1, rr.OBS_COLS)
    M = len(obs)
    d_obs = upload(obs, np.float64) if M else None
    out = Buffers(plan=M * rr.PLAN_COLS * 8, counts=8 * rr.PLAN_COUNTS)
    params = _lib.TrackParams.defaults(max_residual=max_residual)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_object_tracks_suspects(_lib.ptr(d_obs), M, int(T), ctypes.byref(params), out.at("plan") if M else None, out.at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    plan = td._rows(out.raw("plan"), rr.PLAN_COLS, M, "d_plan")
    return plan, out.raw("counts").view(np.int64).copy(), out.raw("plan").tobytes() + out.raw("counts").tobytes()


def check_plan(obs, T, max_residual=0.2, label="", stream=None):
    plan, counts, raw = run_plan(obs, T, max_residual, stream)
    want, want_counts = rr.plan(obs, T, max_residual)
    same(plan, want, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return plan, counts, raw


SELECT_INPUTS = ("T_new", "T_old", "errors", "ious", "translations", "rotations", "errors_old", "centre", "pred")


def run_select(table, iters, params=None, stream=None):
    """One call of icpflow_pairs_repair_select on a dict of numpy arrays (repair_cases.stack) -> (T_out [K, 16], report [K, 12],
    counts [8], the outputs' bytes)"""
    from icp_flow_amd import _lib
    L = _lib._L
    K = len(table["T_new"])
    dev = {k: upload(table[k], np.float64 if k in ("centre", "pred") else F) if K else None for k in SELECT_INPUTS}
    d_iters = upload(np.array([iters], np.int32), np.int32)
    out = Buffers(T_out=K * 64, report=K * rr.REPAIR_COLS * 8, counts=8 * rr.REPAIR_COUNTS)
    p = _lib.RepairParams.defaults(**(params or {}))
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_pairs_repair_select(*(_lib.ptr(dev[k]) for k in ("T_new", "T_old")), _lib.ptr(d_iters) if K else None,
                                           *(_lib.ptr(dev[k]) for k in SELECT_INPUTS[2:]), K, ctypes.byref(p), out.at("T_out") if K else None,
                                           out.at("report") if K else None, out.at("counts"), _lib.stream(DEV))
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    out.check()
    report = td._rows(out.raw("report"), rr.REPAIR_COLS, K, "d_report")
    return (out.raw("T_out").view(F).reshape(K, 16).copy(), report, out.raw("counts").view(np.int64).copy(),
            b"".join(out.raw(k).tobytes() for k in sorted(out.sizes)))


def check_select(table, iters, params=None, label="", stream=None):
    T_out, report, counts, raw = run_select(table, iters, params, stream)
    want_T, want_report, want_counts = rr.select(iters=iters, **table, **(params or {}))
    assert T_out.tobytes() == want_T.tobytes(), (label, "d_T_out")            # bit for bit, a NaN's payload included
    same(report, want_report, label)
    assert np.array_equal(counts, want_counts), (label, counts, want_counts)
    return T_out, report, counts, raw


def pair_clouds(K, seed, lo=60, hi=1100):
    """K rigid pairs: source clusters of lo..hi points on box faces, destination = source moved by up to 0.6 m and turned by a
    few degrees, plus noise; labels 0 .. K - 1 in both clouds, rows shuffled.  -> dict(src, dst [n, 3], labels_src, labels_dst,
    moves [K, 3])"""
    rng = np.random.default_rng(seed)
    src, dst, ls, ld, moves = [], [], [], [], []
    sizes = np.linspace(lo, hi, K).astype(int) if K > 1 else np.array([hi])
    for k, n in enumerate(sizes):
        local = rng.uniform(-1, 1, (n, 3)) * (2.0, 0.8, 0.5)
        face = rng.integers(0, 2, n)                          # every point on a face along x or y
        local[face == 0, 0] = np.sign(local[face == 0, 0]) * 2.0
        local[face == 1, 1] = np.sign(local[face == 1, 1]) * 0.8
        centre = np.array([12.0 * (k % 6), 12.0 * (k // 6), 1.0])
        move, yaw = rng.uniform(-0.35, 0.35, 3) * (1, 1, 0.1), np.deg2rad(rng.uniform(-3, 3))
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        m = max(lo, int(n * rng.uniform(0.8, 1.0)))
        src.append(local + centre)
        dst.append((local[rng.permutation(n)[:m]] @ R.T) + centre + move + rng.normal(0, 0.005, (m, 3)))
        ls.append(np.full(n, k)), ld.append(np.full(m, k)), moves.append(move)
    src, dst, ls, ld = (np.concatenate(x) for x in (src, dst, ls, ld))
    a, b = rng.permutation(len(src)), rng.permutation(len(dst))
    return dict(src=src[a].astype(F), dst=dst[b].astype(F), labels_src=ls[a].astype(F), labels_dst=ld[b].astype(F), moves=np.array(moves))


REG = SimpleNamespace(thres_dist=0.1, icp_max_iterations=100, icp_relative_rmse_thr=1e-6, icp_stop_mode="reference")


def run_reregister(case, N, T_old, pred, params=None, stream=None, K=None):
    """One call of icpflow_pairs_reregister on pair_clouds' case, pair k = cluster k of both clouds, from [I | pred].
    -> dict(T_out, report, counts, clouds [2, K, N, 4] (device), words: the workspace's first region (float32), raw)"""
    from icp_flow_amd import _lib
    L = _lib._L
    K = len(case["moves"]) if K is None else K
    Lmax = 64
    tabs = [bd.cluster_table(case[p], case[lab], Lmax) for p, lab in (("src", "labels_src"), ("dst", "labels_dst"))]
    pts = [upload(case[p], F) for p in ("src", "dst")]
    seg = np.zeros((2, 3, max(K, 1)), np.int64)
    centre = np.zeros((max(K, 1), 3))
    for side, (order, table, num) in enumerate(tabs):
        rows = table.cpu().numpy()[: int(num.item())]
        assert rows[:K, 0].tolist() == list(range(K)) and (rows[:K, 1] <= N).all()
        seg[side, 0, :K], seg[side, 1, :K], seg[side, 2] = rows[:K, 2], rows[:K, 1], -1
        if side == 0:
            centre[:K] = rows[:K, 3:6]
    tables = _lib.Tables(pts[0].data_ptr(), tabs[0][0].data_ptr(), tabs[0][1].data_ptr(), pts[1].data_ptr(), tabs[1][0].data_ptr(), tabs[1][1].data_ptr(),
                         K, K, 9)
    init = np.tile(np.eye(4, dtype=F), (max(K, 1), 1, 1))
    init[:K, :3, 3] = np.asarray(pred, np.float64).reshape(-1, 3)[:K]
    d = dict(seg=upload(seg[:, :, :K] if K else seg, np.int64), init=upload(init, F), T_old=upload(np.asarray(T_old, F).reshape(-1, 16), F),
             centre=upload(centre, np.float64), pred=upload(np.asarray(pred, np.float64).reshape(-1, 3), np.float64))
    need = int(L.icpflow_pairs_reregister_workspace_bytes(K, N))
    assert (need > 0 and need % 256 == 0) if K else need == 0
    ws = rd._guarded(max(need, 256), WS_POISON)
    out = Buffers(clouds=2 * K * N * 16, T_out=K * 64, report=K * rr.REPAIR_COLS * 8, counts=8 * rr.REPAIR_COUNTS)
    p = _lib.RepairParams.defaults(**(params or {}))
    reg = _lib.Registration(None, None, None, 0, 0, 0, 0.0, REG.thres_dist, REG.icp_relative_rmse_thr, REG.icp_max_iterations, 0)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rc = L.icpflow_pairs_reregister(ctypes.byref(tables), K, N, _lib.ptr(d["seg"]), out.at("clouds"), _lib.ptr(d["init"]), _lib.ptr(d["T_old"]),
                                        _lib.ptr(d["centre"]), _lib.ptr(d["pred"]), ctypes.byref(reg), ctypes.byref(p), out.at("T_out"), out.at("report"),
                                        out.at("counts"), ctypes.c_void_p(ws.data_ptr() + GUARD) if K else None, ctypes.c_size_t(need), _lib.stream(DEV), None)
    msg = L.icpflow_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, (rc, msg)
    assert rd._guards_intact(ws, max(need, 256)), "guard of the workspace changed"
    out.check()
    report = td._rows(out.raw("report"), rr.REPAIR_COLS, K, "d_report")
    words = ws[GUARD: GUARD + 4 * (44 * K + 1)].clone().view(torch.float32) if K else None
    clouds = out.bufs["clouds"][GUARD: GUARD + out.sizes["clouds"]].clone().view(torch.float32).reshape(2, K, N, 4) if K else None
    return dict(T_out=out.raw("T_out").view(F).reshape(K, 16).copy(), report=report, counts=out.raw("counts").view(np.int64).copy(), clouds=clouds,
                words=words, init=d["init"], T_old=d["T_old"], centre=centre[:K], pred=np.asarray(pred, np.float64).reshape(-1, 3)[:K],
                raw=b"".join(out.raw(k).tobytes() for k in ("T_out", "report", "counts")))


def split_words(words, K):
    """the workspace's first region -> dict of numpy arrays: T_new [K, 16], the six metric arrays of the new and of the old pose,
    the iteration count"""
    w = words.cpu().numpy()
    cols = (("T_new", 16), ("errors", 2), ("inliers", 2), ("ratios", 2), ("ious", 2), ("translations", 3), ("rotations", 3), ("errors_old", 2),
            ("inliers_old", 2), ("ratios_old", 2), ("ious_old", 2), ("translations_old", 3), ("rotations_old", 3))
    out, at = {}, 0
    for name, c in cols:
        out[name], at = w[at: at + c * K].reshape(K, c).copy(), at + c * K
    out["iters"] = int(w[at:].view(np.int32)[0])
    return out

"""Judges of a registered frame pair that need no ground truth, and the shape run_stream gives them.

The device functions take a FramePair and what its registration returned (dict(pairs, transformations, flow, ...)):
`frame_residual` (the nearest-neighbour residual, icpflow_nn_residual), `frame_segment_residual` (per segment of the source),
`frame_segment_sight` (with the line of sight beside it, icpflow_sight_*), `frame_trust` (one trust byte per source point),
`frame_objects` (a box and a velocity per matched pair), `frame_tracks` (a sample's objects linked across its gaps) and
`log_tracks` (a log's objects linked from file to file); the `residual_*` helpers carry the residual's tables through the all_reduce and in and out of the summary's block.

Below them one plain class per judge: its constructor reads its attributes of `args` and raises on a bad combination,
`account(number, fp, out)` judges one registered frame pair (`timed` brackets the device work), `summarise(out)` adds its keys
to the summary and writes its file; the residual alone has `reduce_words` / `take_words`, its ride on the closing all_reduce.
The log's tracks alone have `close`, called once the stream's last frame pair is accounted.  frame_pairs.run_stream builds the
seven in one place and calls them in that order; what one judge needs of another is a constructor argument."""
import contextlib
import json
import time

import numpy as np
import torch

from . import utils_check, utils_eval, utils_flow, utils_objects, utils_tracks
from .pair_data import _input


def residual_groups(labels_src, pairs):
    """The group of every source row for the residual's table (utils_eval.RESIDUAL_GROUPS): 0 ground (label -1e8), 1 unclustered
    (-1), 2 clustered but unmatched, 3 matched -- its label is the source label of a row of `pairs` ([P,10], column 0).  Device
    tensors in, int32 [Ns] on the device out."""
    matched = torch.isin(labels_src, pairs[:, 0].to(labels_src.dtype)) if pairs.shape[0] else torch.zeros_like(labels_src, dtype=torch.bool)
    g = torch.where(matched, 3, 2).to(torch.int32)
    g = torch.where(labels_src == -1.0, torch.ones_like(g), g)
    return torch.where(labels_src == -1e8, torch.zeros_like(g), g).contiguous()


def frame_residual(fp, out, device, radius, edges=utils_eval.RESIDUAL_EDGES):
    """The four residual calls of one registered frame pair and their one read-back: AFTER (the flow's source points -- raw when
    the pair carries them -- plus the predicted flow against the destination, and the destination against that warped cloud) and
    BEFORE (the ego-compensated source against the destination with no flow, and back).  The source's rows are grouped by
    `residual_groups`, the destination's form one group.  -> [after forward, after backward, before forward, before backward],
    ResidualTables."""
    device = torch.device(device)
    ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
    raw = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
    groups = residual_groups(_source_labels(fp, out, device), out["pairs"].to(device))
    flow = out["flow"].to(device).float()
    G = len(utils_eval.RESIDUAL_GROUPS)
    calls = ((raw, pd, flow, groups, G), (pd, raw[:, 0:3] + flow[:, 0:3], None, None, 1), (ps, pd, None, groups, G), (pd, ps, None, None, 1))
    words = [utils_eval.nn_residual_device(q, t, f, radius, g, n, edges, per_row=False)[2] for q, t, f, g, n in calls]
    host = torch.cat(words).cpu().numpy()             # the one read-back
    tables, at = [], 0
    for _, _, _, _, n in calls:
        size = n * (len(edges) + 4)
        tables.append(utils_eval.ResidualTable.from_words(host[at: at + size], n, tuple(edges), radius, bad=int(host[at + size])))
        at += size + 4
    return tables


def _source_labels(fp, out, device):
    ls = out.get("labels_src")
    if ls is None and fp.labels_src is not None:
        ls = _input(fp, "labels_src", device)
    if ls is None:
        raise ValueError("the residual groups the source rows by their cluster labels: the registration must leave labels_src in its result")
    return ls.to(device).float()


def frame_segment_residual(fp, out, device, radius, edges=utils_eval.RESIDUAL_EDGES):
    """The residual of one registered frame pair PER SEGMENT of the source (utils_eval.segment_residual: one call, one
    read-back): BEFORE the ego-compensated source, AFTER the flow's source points -- raw when the pair carries them -- plus the
    predicted flow, both against the destination; the source labels as `frame_residual` finds them.  -> SegmentResidual"""
    device = torch.device(device)
    ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
    raw = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
    return utils_eval.segment_residual(ps, raw, out["flow"].to(device).float(), _source_labels(fp, out, device), pd, radius, edges)


def frame_segment_sight(fp, out, device, radius, origin=(0.0, 0.0, 0.0), edges=utils_eval.RESIDUAL_EDGES, **params):
    """`frame_segment_residual` with the line-of-sight check beside it (utils_eval.segment_sight): the same residual call with
    its per-row distances kept, one depth image over the destination as seen from `origin`, and the codes per segment among
    the rows further than RESIDUAL_EDGES[1] metres from every destination point.  -> (SegmentResidual, sight), `sight` a
    function without arguments that enqueues the image and the table and reads the table back -> SegmentSight (run_stream
    times the two parts apart)."""
    device = torch.device(device)
    ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
    raw = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
    flow, labels = out["flow"].to(device).float(), _source_labels(fp, out, device)
    table, num, info, d2b, d2a = utils_eval.segment_residual_device(ps, raw, flow, labels, pd, radius, edges, per_row=True)
    report = utils_eval.segment_residual_read(table, num, info, radius, edges)

    def sight():
        image = utils_eval.sight_image(pd, origin, **params)
        return utils_eval.segment_sight(image, ps, raw, flow, labels, d2b, d2a, far=utils_eval.RESIDUAL_EDGES[1])

    return report, sight


def frame_trust(fp, out, device, radius, origin=None, params=None):
    """One trust byte per source point of a registered frame pair (utils_eval.flow_trust_device), everything on the device: the
    segments' residual with its per-row distances kept (`frame_segment_residual`'s call), with an `origin` the depth image over
    the destination and the segments' line-of-sight table with its per-row codes (`frame_segment_sight`'s calls), then the one
    call that turns the tables and the per-row arrays into bytes.  The far rows and the listing share utils_eval.RESIDUAL_EDGES[1]
    (params: a _lib.TrustParams that says otherwise).  -> (trust uint8 [Ns] on the device, TrustCounts); one read-back, the
    sixteen counts."""
    device = torch.device(device)
    ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
    raw = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
    flow, labels = out["flow"].to(device).float(), _source_labels(fp, out, device)
    far = utils_eval.RESIDUAL_EDGES[1] if params is None else float(params.far)
    table, num, _, d2b, d2a = utils_eval.segment_residual_device(ps, raw, flow, labels, pd, radius, per_row=True)
    seen = code = None
    if origin is not None:
        image = utils_eval.sight_image(pd, origin)
        seen, _, _, _, code = utils_eval.segment_sight_device(image, ps, raw, flow, labels, d2b, d2a, far=far, per_row=True)
    trust, _, counts = utils_eval.flow_trust_device(raw, flow, labels, table, num, d2a, out["pairs"].to(device), seen, code, params)
    return trust, utils_eval.TrustCounts(counts.cpu().numpy())     # the one read-back


def frame_objects(fp, out, device, seconds=None, min_speed=utils_objects.MIN_SPEED, delta=utils_objects.BOX_DELTA, A=utils_objects.BOX_DIRECTIONS):
    """One object row per matched pair of a registered frame pair (utils_objects), everything on the device: the boxes of the
    ego-compensated source's clusters and of the destination's (the cloud the pairs' transforms register, and the one they
    register it to), then a box, a displacement, a velocity and a heading per pair from `out`'s pair rows and transforms.
    seconds: the time between the two sweeps (None: fp.gap sweeps of utils_objects.SWEEP_SECONDS).  -> utils_objects.Objects;
    one read-back, the pairs' table with its four counts."""
    seconds = float(fp.gap) * utils_objects.SWEEP_SECONDS if seconds is None else float(seconds)
    rows, counts, _ = _frame_objects_device(fp, out, device, seconds, min_speed, delta, A)
    return utils_objects.Objects.read(rows, counts, seconds, min_speed)     # the one read-back


def _frame_objects_device(fp, out, device, seconds, min_speed, delta=utils_objects.BOX_DELTA, A=utils_objects.BOX_DIRECTIONS, boxes=False):
    """frame_objects' three calls, nothing read back -> (rows float64 [P, 24], counts int64 [4], the destination's labels); with
    `boxes` a fourth: (the source's box table, its number), as the first call left them"""
    device = torch.device(device)
    ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
    ls = _source_labels(fp, out, device)
    ld = out.get("labels_dst")
    if ld is None and fp.labels_dst is not None:
        ld = _input(fp, "labels_dst", device)
    if ld is None:
        raise ValueError("the objects need the destination's cluster labels: the registration must leave labels_dst in its result")
    ld = ld.to(device).float()
    boxes_src, num_src = utils_objects.segment_boxes_device(ps, ls, delta, A)
    boxes_dst, num_dst = utils_objects.segment_boxes_device(pd, ld, delta, A)
    rows, counts = utils_objects.pair_objects_device(boxes_src, num_src, out["pairs"].to(device), out["transformations"].to(device),
                                                     boxes_dst, num_dst, seconds, min_speed)
    return (rows, counts, ld, (boxes_src, num_src)) if boxes else (rows, counts, ld)


def frame_tracks(fps, outs, device, sweep_seconds=utils_objects.SWEEP_SECONDS, min_speed=utils_tracks.MIN_SPEED, min_iou=utils_tracks.MIN_IOU,
                 max_residual=utils_tracks.MAX_RESIDUAL, Lmax=4096, repair=False, args=None, fill=False):
    """The object tracks of ONE sample (utils_tracks), everything on the device: `fps` the sample's frame pairs in gap order --
    they share the destination sweep, row for row -- and `outs` their registrations.  Per gap the object rows of frame_objects
    (not read back), then the shared sweep's clusters linked to the tracks so far (icpflow_object_tracks_extend); at the end one
    fit over all gaps and ONE read-back.  A gap of `gap` sweeps spans gap * sweep_seconds.  -> utils_tracks.Tracks

    repair=True (with `args`, what the frame pairs were registered with): the gaps that alone break a track's constant velocity
    are registered again (include/icpflow_hip.h, 8(m)).  After the tracks as above, icpflow_object_tracks_suspects over all
    observations and its one read-back (with the pairs' labels); a sample without a suspect launches nothing more.  Per gap with
    suspects one icpflow_pairs_reregister from the pure translations the other gaps predict -- a pair with a cluster longer than
    args.max_points is not retried (reason 6: its subsample would draw random numbers); every `out` of such a gap gets NEW
    tensors under `transformations` (the accepted poses in their rows), `pairs` (their error, inlier, ratio and iou columns from
    the new metrics) and `flow` (utils_flow.flow_estimation_torch on the patched rows); then the object rows and the tracks are
    computed again.  -> the Tracks after repair, its `repair` a utils_tracks.Repair (the Tracks before, the retried pairs).

    fill=True (with `args`; after the repair when both are asked for, on the repaired tracks): the gaps in which a track found no
    pair are registered from what the other gaps predict (include/icpflow_hip.h, 8(n)).  icpflow_object_tracks_missing over all
    gap slots; its missing rows are compacted on the device and read back once with the counts (FILL_READ_ROWS of them; a sample
    with more reads a second time); a sample without a missing row launches nothing more.  Per gap with missing rows
    icpflow_pairs_fill_candidates on that gap's source boxes (the chain's own, not computed twice) and one read-back of every
    choice; a chosen pair with a destination cluster longer than args.max_points is left out (reason 6); the others are registered
    by icpflow_pairs_reregister from [I | p] with T_old = identity, so the select's reason 4 compares the new pose with the ego
    motion alone on the same clouds.  Accepted pairs are APPENDED, in ascending plan-row order, to NEW tensors under `pairs`
    (the chosen source label, the plan's destination label, then the new metrics in the repair's order) and `transformations`
    of that gap's `out` -- the old rows keep every bit --, `flow` is computed again, and so are the object rows and the tracks.
    -> the Tracks after the fill, its `fill` a utils_tracks.Fill (the Tracks before, one entry per missing row)."""
    device = torch.device(device)
    n = len(fps[0].points_dst)
    if any(len(fp.points_dst) != n for fp in fps):
        raise ValueError(f"object tracks: the frame pairs of {fps[0].sequence or fps[0].name!r} disagree on the rows of the shared sweep "
                         f"({sorted({len(fp.points_dst) for fp in fps})}): they are not the gaps of one sample")

    def chain():
        state, tables, boxes = utils_tracks.TrackState(n, device, Lmax, min_iou, max_residual, min_speed), [], []
        for fp, out in zip(fps, outs):
            seconds = float(fp.gap) * float(sweep_seconds)
            rows, _, ld, box = _frame_objects_device(fp, out, device, seconds, min_speed, boxes=True)
            state.extend(ld, rows, fp.gap, seconds)
            tables.append(rows), boxes.append(box)
        state.fit()
        return state, tables, boxes

    state, tables, boxes = chain()
    if not repair and not fill:
        return state.read()
    if args is None:
        raise ValueError(f"frame_tracks({'repair' if repair else 'fill'}=True) registers again: it needs the `args` the frame pairs were registered with")
    if repair:
        after, state, tables, boxes = _repair_tracks(fps, outs, device, args, max_residual, state, tables, boxes, chain)
    else:
        after = state.read()
    if fill:
        after = _fill_tracks(fps, outs, device, args, max_residual, [float(fp.gap) * float(sweep_seconds) for fp in fps], state, boxes, chain, after)
    return after


def _repair_tracks(fps, outs, device, args, max_residual, state, tables, boxes, chain):
    """frame_tracks(repair=True) behind the first chain -> (the Tracks after repair, and the state, object tables and source boxes
    they were computed from: the second chain's where a pair was retried)"""
    plan, plan_counts = utils_tracks.suspects_device(torch.cat(state.obs), state.bound, max_residual)
    before = state.read()
    t0 = time.perf_counter()                                 # (the read-back above left the stream empty; the last one below drains it)
    sizes = [int(t.shape[0]) for t in tables]
    labels = [out["pairs"][:, 0:2].to(device=device, dtype=torch.float64).reshape(-1) for out in outs]
    host = torch.cat([plan_counts.to(torch.float64), plan.reshape(-1)] + labels).cpu().numpy()        # the plan's one read-back
    plan_counts, at = np.rint(host[:4]).astype(np.int64), 4 + 8 * sum(sizes)
    h_plan = host[4: at].reshape(-1, 8)
    retried, counts, results, first = [], np.zeros(8, np.int64), [], 0
    for g, (fp, out, rows, P) in enumerate(zip(fps, outs, tables, sizes)):
        pair_labels, at = host[at: at + 2 * P].reshape(P, 2), at + 2 * P
        mine, first = np.flatnonzero(h_plan[first: first + P, 0] == 1.0), first + P
        if len(mine) == 0:
            continue
        ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
        ls, ld = _source_labels(fp, out, device), out["labels_dst"].to(device).float() if out.get("labels_dst") is not None else _input(fp, "labels_dst", device).float()
        st, dt = utils_check.ClusterTable.pair(ps, ls, pd, ld)
        si, di = st.find_host(pair_labels[mine, 0]), dt.find_host(pair_labels[mine, 1])
        fits = (si >= 0) & (di >= 0)
        fits[fits] = (st.h_count[si[fits]] <= int(args.max_points)) & (dt.h_count[di[fits]] <= int(args.max_points))
        entry = lambda p, g=g, pair_labels=pair_labels: dict(gap=g, pair=int(p), labels=[float(v) for v in pair_labels[p]], track=int(before.observation_ids[g][p]))   # noqa: E731
        for p in mine[~fits]:
            retried.append(dict(entry(p), reason=utils_tracks.REPAIR_TOO_LONG, accepted=False))
            counts[utils_tracks.REPAIR_TOO_LONG] += 1
        mine, si, di = mine[fits], si[fits], di[fits]
        if len(mine) == 0:
            continue
        idx = torch.from_numpy(mine).to(device)
        T = out["transformations"].to(device=device, dtype=torch.float32).reshape(P, 16)
        params = utils_tracks.repair_params(args, out["translation_frame"], max_residual)
        res = utils_tracks.reregister_device(args, st, dt, si, di, T[idx], rows[idx, 4:7], plan[first - P + idx, 3:6], params)
        T, pairs = T.clone(), out["pairs"].to(device).clone()
        T[idx] = res["T"].reshape(-1, 16)                       # (a rejected pair's row is its old one, bit for bit)
        fresh = torch.cat([res["errors"], res["inliers"], res["ratios"], res["ious"]], dim=1)
        pairs[idx, 2:10] = torch.where(res["report"][:, 11:12] == 1.0, fresh, pairs[idx, 2:10])
        out["pairs"], out["transformations"] = pairs, T.view(P, 4, 4)
        flow_src = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
        out["flow"] = utils_flow.flow_estimation_torch(args, flow_src, pd, ls, ld, pairs, out["transformations"], torch.from_numpy(fp.pose).to(device))
        results.append((mine, entry, res))
    if results:
        host = torch.cat([torch.cat([r["counts"].to(torch.float64), r["report"].reshape(-1)]) for _, _, r in results]).cpu().numpy()
        at = 0
        for mine, entry, _ in results:
            counts += np.rint(host[at: at + 8]).astype(np.int64)
            report, at = host[at + 8: at + 8 + 12 * len(mine)].reshape(-1, 12), at + 8 + 12 * len(mine)
            for p, r in zip(mine, report):
                retried.append(dict(entry(p), reason=int(r[0]), e_old=float(r[2]), e_new=float(r[1]), distance=float(r[6]), accepted=bool(r[11])))
        state, tables, boxes = chain()                       # the object rows and the tracks, again, on the repaired gaps
    after = state.read() if results else before
    after.repair = utils_tracks.Repair(before, plan_counts, sorted(retried, key=lambda e: (e["gap"], e["pair"])), counts, (time.perf_counter() - t0) * 1e3)
    return after, state, tables, boxes


FILL_READ_ROWS = 1024            # missing rows the plan's one read-back has room for; a sample with more reads the plan a second time


def _fill_tracks(fps, outs, device, args, max_residual, seconds, state, boxes, chain, before):
    """frame_tracks(fill=True) behind the chain (and the repair) -> the Tracks after the fill, its `fill` a utils_tracks.Fill;
    `before`: the Tracks read from `state`"""
    t0 = time.perf_counter()                                 # (the tracks' read-back left the stream empty; the last one below drains it)
    R, f64 = utils_tracks.FILL_REASONS, torch.float64
    segments, nums = torch.stack([s for s, _ in state.segments]), torch.cat([k for _, k in state.segments])
    G, Lmax = int(segments.shape[0]), int(segments.shape[1])
    plan, plan_counts = utils_tracks.missing_device(torch.cat(state.obs), state.bound, segments, nums, state.gaps, seconds, max_residual)
    flat = plan.view(G * Lmax, -1)
    cap = min(G * Lmax, FILL_READ_ROWS)
    first = torch.argsort(flat[:, 0], descending=True, stable=True)[:cap]     # the missing rows first, in ascending plan-row order
    host = torch.cat([plan_counts.to(f64).reshape(-1), first.to(f64), flat[first].reshape(-1)]).cpu().numpy()   # the plan's one read-back
    plan_counts = np.rint(host[: 4 * G]).astype(np.int64).reshape(G, 4).sum(axis=0)
    K = int(plan_counts[3])
    if K > cap:
        first = torch.argsort(flat[:, 0], descending=True, stable=True)[:K]
        host = np.concatenate([host[: 4 * G], torch.cat([first.to(f64), flat[first].reshape(-1)]).cpu().numpy()])
        cap = K
    where = np.rint(host[4 * G: 4 * G + cap]).astype(np.int64)[:K]
    h_plan = host[4 * G + cap:].reshape(cap, -1)[:K]
    counts, entries = np.zeros(len(R), np.int64), []
    for w, r in zip(where, h_plan):
        entries.append(dict(gap=int(w // Lmax), segment=int(w % Lmax), track=int(r[1]), labels=[None, float(r[2])], reason=None, accepted=False, pair=None))
    by_gap = {g: [k for k, e in enumerate(entries) if e["gap"] == g] for g in sorted({e["gap"] for e in entries})}
    # the candidates of every gap with missing rows, and their one read-back
    chosen = {}
    for g, ks in by_gap.items():
        q = flat[torch.from_numpy(where[ks]).to(device), 9:12]
        chosen[g] = utils_tracks.fill_candidates_device(q, boxes[g][0], boxes[g][1], outs[g]["pairs"].to(device), utils_tracks.FILL_RADIUS, int(args.max_points))[0]
    h_choice = torch.cat([chosen[g].reshape(-1) for g in by_gap]).cpu().numpy().reshape(-1, 8) if by_gap else np.zeros((0, 8))
    results, at = [], 0
    for g, ks in by_gap.items():
        fp, out = fps[g], outs[g]
        choice, at = h_choice[at: at + len(ks)], at + len(ks)
        for k, c in zip(ks, choice):
            if c[0] != 0.0:
                entries[k]["reason"] = utils_tracks.FILL_NO_CANDIDATE if c[0] == 1.0 else utils_tracks.FILL_LOST
                counts[entries[k]["reason"]] += 1
            else:
                entries[k]["labels"][0] = float(c[2])
        live = [j for j, c in enumerate(choice) if c[0] == 0.0]
        if not live:
            continue
        ps, pd = _input(fp, "points_src", device), _input(fp, "points_dst", device)
        ls, ld = _source_labels(fp, out, device), out["labels_dst"].to(device).float() if out.get("labels_dst") is not None else _input(fp, "labels_dst", device).float()
        st, dt = utils_check.ClusterTable.pair(ps, ls, pd, ld)
        si, di = st.find_host(choice[live, 2]), dt.find_host(h_plan[np.asarray(ks)[live], 2])
        fits = (si >= 0) & (di >= 0)
        fits[fits] = (st.h_count[si[fits]] <= int(args.max_points)) & (dt.h_count[di[fits]] <= int(args.max_points))
        for j in np.asarray(live)[~fits]:
            entries[ks[j]]["reason"] = utils_tracks.REPAIR_TOO_LONG
            counts[utils_tracks.REPAIR_TOO_LONG] += 1
        live, si, di = np.asarray(live)[fits], si[fits], di[fits]
        if len(live) == 0:
            continue
        rows = torch.from_numpy(where[np.asarray(ks)[live]]).to(device)
        centre = torch.from_numpy(np.ascontiguousarray(choice[live, 5:8])).to(device)
        unmoved = torch.eye(4, dtype=torch.float32, device=device).repeat(len(live), 1, 1)      # T_old: the ego motion alone, what the flow gave the cluster
        params = utils_tracks.repair_params(args, out["translation_frame"], max_residual)
        res = utils_tracks.reregister_device(args, st, dt, si, di, unmoved, centre, flat[rows, 6:9], params)
        results.append((g, [ks[j] for j in live], res, (ps, pd, ls, ld)))
    filled = False
    if results:
        host = torch.cat([torch.cat([r["counts"].to(f64), r["report"].reshape(-1)]) for _, _, r, _ in results]).cpu().numpy()
        at = 0
        for g, ks, res, (ps, pd, ls, ld) in results:
            fp, out = fps[g], outs[g]
            counts[:8] += np.rint(host[at: at + 8]).astype(np.int64)
            report, at = host[at + 8: at + 8 + 12 * len(ks)].reshape(-1, 12), at + 8 + 12 * len(ks)
            pairs, T = out["pairs"].to(device), out["transformations"].to(device)
            P = int(pairs.shape[0])
            for k, r in zip(ks, report):
                entries[k].update(reason=int(r[0]), e_old=float(r[2]), e_new=float(r[1]), distance=float(r[6]), accepted=bool(r[11]))
            took = [j for j, r in enumerate(report) if r[11] == 1.0]
            if not took:
                continue
            for row, j in enumerate(took):
                entries[ks[j]]["pair"] = P + row
            idx = torch.from_numpy(np.asarray(took, np.int64)).to(device)
            labels = torch.tensor([entries[ks[j]]["labels"] for j in took], dtype=torch.float64, device=device)
            fresh = torch.cat([labels.to(pairs.dtype), res["errors"][idx].to(pairs.dtype), res["inliers"][idx].to(pairs.dtype),
                               res["ratios"][idx].to(pairs.dtype), res["ious"][idx].to(pairs.dtype)], dim=1)
            out["pairs"] = torch.cat([pairs.reshape(P, -1), fresh])              # NEW tensors: the old rows keep every bit
            out["transformations"] = torch.cat([T.reshape(P, 4, 4), res["T"][idx].to(T.dtype).reshape(-1, 4, 4)])
            flow_src = ps if fp.points_src_raw is None else _input(fp, "points_src_raw", device)
            out["flow"] = utils_flow.flow_estimation_torch(args, flow_src, pd, ls, ld, out["pairs"], out["transformations"], torch.from_numpy(fp.pose).to(device))
            filled = True
    if filled:
        state, _, _ = chain()                                # the object rows and the tracks, again, on the filled gaps
    after = state.read() if filled else before
    after.repair = before.repair
    after.fill = utils_tracks.Fill(before, plan_counts, entries, counts, (time.perf_counter() - t0) * 1e3)
    return after


def log_frames(poses):
    """The frames of a log's files for icpflow_object_tracks_path, on the host in float64: file k's destination frame into the
    log's frame (file 0's destination frame).  poses: FramePair.pose_exact of every file, in order -- pose k carries sweep k's
    frame into sweep k + 1's.  W_0 = I, W_{k+1} = W_k inverse(pose_{k+1}), the inverse of a rigid pose (R, t) being (R^T, -R^T t).
    -> float64 [F, 12]: the rotation row-major, then the translation"""
    W, out = np.eye(4), []
    for k, pose in enumerate(poses):
        if k > 0:
            P = np.asarray(pose, np.float64).reshape(4, 4)
            inv = np.eye(4)
            inv[:3, :3] = P[:3, :3].T
            inv[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
            W = W @ inv
        out.append(np.concatenate([W[:3, :3].reshape(9), W[:3, 3]]))
    return np.array(out, np.float64).reshape(len(out), 12)


class LogChain:
    """The object tracks of ONE log (utils_tracks, include/icpflow_hip.h 8(l)), everything on the device: `add` takes the log's
    registered frame pairs in file order -- file k registers sweep k onto sweep k + 1, so the destination of one file is the
    source of the next, in another frame and with other rows.  Per file: the ids of the previous file's destination rows are
    carried onto this file's source rows by nearest rows under this file's pose (icpflow_rows_carry; all -1 for the first file
    or after a break), the source clusters are linked to them (icpflow_object_tracks_extend_side, side 0, one running id
    counter), and the destination rows take the ids of their pairs (icpflow_pair_row_ids), kept with the destination points
    for the next file -- nothing older is kept.  `read` closes the log: one icpflow_object_tracks_path and ONE read-back."""

    def __init__(self, device, sweep_seconds=utils_objects.SWEEP_SECONDS, min_speed=utils_tracks.MIN_SPEED, min_iou=utils_tracks.MIN_IOU,
                 radius=utils_tracks.CARRY_RADIUS, min_share=utils_tracks.CARRY_MIN_SHARE, max_dv=utils_tracks.MAX_DV, Lmax=4096):
        from . import _lib
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("icp_flow_amd: the tracks live on a GPU (HIP) device -- there is no CPU path")
        self.sweep_seconds, self.min_speed, self.min_iou, self.Lmax = float(sweep_seconds), float(min_speed), float(min_iou), int(Lmax)
        self.radius, self.min_share = float(radius), float(min_share)
        self.params = _lib.TrackPathParams.defaults(max_dv=max_dv, min_speed=min_speed)
        self.next_id = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.bound = 0                           # no track id reaches this
        self.last = None                         # (points_dst, the ids of its rows) of the file before
        self.obs, self.carry_counts, self.extend_counts, self.poses, self.names, self.source_rows = [], [], [], [], [], []

    def add(self, fp, out):
        """one file, enqueued on the current stream; nothing is read back"""
        device = self.device
        seconds = float(fp.gap) * self.sweep_seconds
        rows, _, ld = _frame_objects_device(fp, out, device, seconds, self.min_speed)
        ps, pd, ls = _input(fp, "points_src", device), _input(fp, "points_dst", device), _source_labels(fp, out, device)
        n = int(ps.shape[0])
        if self.last is None:
            prior = torch.full((n,), -1, dtype=torch.int32, device=device)
            carried = torch.zeros(6, dtype=torch.int64, device=device)
        else:
            prior, carried = utils_tracks.rows_carry_device(self.last[0], self.last[1], fp.pose_exact, ps, self.radius, self.min_share)
        state = utils_tracks.TrackState(n, device, self.Lmax, self.min_iou, min_speed=self.min_speed, track_of_row=prior, next_id=self.next_id,
                                        bound=self.bound)
        _, _, obs, counts = state.extend(ls, rows, 0, seconds, side=0)
        self.bound = state.bound
        weight = rows[:, 22] if rows.shape[0] else None       # the pairs' source points: a strided view, taken as it is
        ids, _ = utils_tracks.pair_row_ids_device(ld, out["pairs"].to(device), 1, obs[:, 0].to(torch.int32), weight)
        self.last = (pd, ids)
        self.obs.append(obs), self.carry_counts.append(carried), self.extend_counts.append(counts)
        self.poses.append(np.asarray(fp.pose_exact, np.float64)), self.names.append(fp.name), self.source_rows.append(n)

    def read(self):
        """-> utils_tracks.LogTracks: the table over the whole log, every file's counts and observations in ONE transfer"""
        from . import _lib
        import ctypes
        device, F = self.device, len(self.obs)
        every = torch.cat(self.obs) if self.obs else torch.empty((0, _lib.TRACK_OBS_COLS), dtype=torch.float64, device=device)
        M, T = int(every.shape[0]), self.bound
        step_host = np.repeat(np.arange(F, dtype=np.int32), [int(o.shape[0]) for o in self.obs]) if F else np.zeros(0, np.int32)
        frames_host = log_frames(self.poses)
        step, frames = torch.from_numpy(step_host).to(device), torch.from_numpy(frames_host).to(device)
        paths = torch.empty((T, _lib.TRACK_PATH_COLS), dtype=torch.float64, device=device)
        counts = torch.empty(_lib.TRACK_PATH_COUNTS, dtype=torch.int64, device=device)
        with torch.cuda.device(device):
            _lib.call("icpflow_object_tracks_path", _lib.ptr(every) if M else None, _lib.ptr(step) if M else None, M, _lib.ptr(frames) if F else None, F, T,
                      ctypes.byref(self.params), _lib.ptr(paths) if T else None, _lib.ptr(counts), _lib.stream(device))
        f64 = lambda t: t.to(torch.float64).reshape(-1)     # noqa: E731  (ids and counts are exact in a float64)
        parts = [f64(self.next_id), f64(counts)] + [f64(c) for c in self.carry_counts] + [f64(c) for c in self.extend_counts] + [every.reshape(-1), paths.reshape(-1)]
        host = torch.cat(parts).cpu().numpy()             # the one read-back
        at = 0

        def take(k):
            nonlocal at
            at += k
            return host[at - k: at]

        next_id = int(take(1)[0])
        path_counts = np.rint(take(5)).astype(np.int64)
        carry = [np.rint(take(6)).astype(np.int64) for _ in range(F)]
        extend = [np.rint(take(6)).astype(np.int64) for _ in range(F)]
        table = take(M * 13).reshape(M, 13)
        observations = np.split(table, np.cumsum([int(o.shape[0]) for o in self.obs])[:-1]) if F else []
        rows = take(T * 24).reshape(T, 24)[:next_id]
        path_counts[0] = next_id                        # (the call counted the bound's rows; the tracks are the ids handed out)
        params = dict(self.params.as_dict(), radius=self.radius, min_share=self.min_share, min_iou=self.min_iou, sweep_seconds=self.sweep_seconds)
        return utils_tracks.LogTracks(rows, path_counts, next_id, observations, carry, extend, frames_host, self.names, self.source_rows, params)


def log_tracks(fps, outs, device, sweep_seconds=utils_objects.SWEEP_SECONDS, min_speed=utils_tracks.MIN_SPEED, min_iou=utils_tracks.MIN_IOU,
               radius=utils_tracks.CARRY_RADIUS, min_share=utils_tracks.CARRY_MIN_SHARE, max_dv=utils_tracks.MAX_DV, Lmax=4096):
    """The object tracks of one log: `fps` its frame pairs in file order (the destination sweep of one is the source sweep of the
    next, carried over by the next one's pose) and `outs` their registrations -- `LogChain.add` for each, then its `read`.
    -> utils_tracks.LogTracks"""
    chain = LogChain(device, sweep_seconds, min_speed, min_iou, radius, min_share, max_dv, Lmax)
    for fp, out in zip(fps, outs):
        chain.add(fp, out)
    return chain.read()


RESIDUAL_SEGMENTS_SHOWN = 50     # entries of the summary's `residual_segments` block (the file takes all of them)


def _residual_flat(tables):
    """the four tables as one list of numbers for the closing all_reduce (counts are exact in a float64), and back"""
    flat = []
    for t in tables:
        flat += t.rows.tolist() + t.hits.tolist() + t.under.reshape(-1).tolist() + t.dsum.tolist() + t.ddsum.tolist() + [t.bad]
    return [float(v) for v in flat]


def _residual_unflat(flat, like):
    tables, at = [], 0
    for t in like:
        G, E = len(t.rows), len(t.edges)
        take = lambda k: [flat[at + j] for j in range(k)]   # noqa: E731
        rows = take(G); at += G
        hits = take(G); at += G
        under = take(G * E); at += G * E
        dsum = take(G); at += G
        ddsum = take(G); at += G
        tables.append(utils_eval.ResidualTable(np.rint(rows), np.rint(hits), np.rint(under), dsum, ddsum, t.edges, t.radius, bad=int(round(flat[at]))))
        at += 1
    return tables


def _residual_zero(radius, edges=utils_eval.RESIDUAL_EDGES):
    G = len(utils_eval.RESIDUAL_GROUPS)
    return [utils_eval.ResidualTable.zeros(n, tuple(edges), radius) for n in (G, 1, G, 1)]


def residual_block(tables):
    """[after forward, after backward, before forward, before backward] -> the summary's `residual` block"""
    af, ab, bf, bb = tables
    side = lambda f, b: dict(forward=f.summary(utils_eval.RESIDUAL_GROUPS), backward=b.summary(("all",)), chamfer=f.mean() + b.mean())   # noqa: E731
    words = dict(after_forward=af.words().tolist(), after_backward=ab.words().tolist(), before_forward=bf.words().tolist(),
                 before_backward=bb.words().tolist())      # the tables themselves (ResidualTable.from_words): runs can be added
    return dict(radius=af.radius, edges=list(af.edges), groups=list(utils_eval.RESIDUAL_GROUPS), before=side(bf, bb), after=side(af, ab),
                words=words)


def residual_tables(block):
    """the summary's `residual` block -> (before, after), each dict(forward, backward: ResidualTable), what format_residual takes"""
    edges, r, G = tuple(block["edges"]), block["radius"], len(block["groups"])
    table = lambda key, n: utils_eval.ResidualTable.from_words(block["words"][key], n, edges, r)   # noqa: E731
    return (dict(forward=table("before_forward", G), backward=table("before_backward", 1)),
            dict(forward=table("after_forward", G), backward=table("after_backward", 1)))


@contextlib.contextmanager
def timed(device, sink, settled=False):
    """Synchronise `device`, start the clock, run the body, synchronise, append the milliseconds to `sink`.  settled: the body
    follows a synchronise with nothing enqueued since, and the clock starts without another one."""
    if device.type == "cuda" and not settled:
        torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    yield
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    sink.append((time.perf_counter() - t0) * 1e3)


class ResidualJudge:
    """args.residual = r (metres; `--residual [R]`): every frame pair is also judged WITHOUT ground truth -- `frame_residual`, after
    the pair is registered (and, in flight, delivered) and outside the timed region of one pair at a time; the tables are added
    in the order of the frame pairs whatever order they complete in, ride the closing all_reduce, and the summary gains a
    `residual` block and `ms_residual_per_frame_pair` (device-synchronised around the four calls and their read-back).  In flight,
    ms / frame pair is the wall time of the share and then includes this work."""

    def __init__(self, args, world, device):
        self.radius, self.world, self.device = getattr(args, "residual", None), world, device
        self.on = bool(self.radius)
        self.tables, self.ms = {}, []              # frame pair (its number in this rank's share) -> its four tables

    def account(self, number, fp, out):
        with timed(self.device, self.ms):
            self.tables[number] = frame_residual(fp, out, self.device, float(self.radius))

    def reduce_words(self):
        self.total = _residual_zero(float(self.radius))
        for number in sorted(self.tables):
            for acc, t in zip(self.total, self.tables[number]):
                acc.add(t)
        return [sum(self.ms)] + _residual_flat(self.total)

    def take_words(self, words):
        self.ms_sum = words[0]
        if self.world > 1:
            self.total = _residual_unflat(words[1:], self.total)

    def summarise(self, out):
        out["ms_residual_per_frame_pair"] = self.ms_sum / max(out["frame_pairs"], 1)
        out["residual"] = residual_block(self.total)


class SegmentJudge:
    """args.residual_segments = True or a file name (`--residual-segments [FILE]`; needs args.residual, whose radius it shares; one
    process only): every frame pair is judged PER SEGMENT of its source as well -- `frame_segment_residual`, next to
    `frame_residual` and like it outside the timed region of one pair at a time -- and the segments whose mean distance under the
    flow exceeds utils_eval.RESIDUAL_EDGES[1] metres are collected, worst first.  The summary gains `residual_segments` (above,
    segments_judged, segments_listed, worst: at most RESIDUAL_SEGMENTS_SHOWN entries, each with its frame pair's number and
    path), `ms_segment_residual_per_frame_pair` (device-synchronised around the call and its read-back) and, with a file name,
    `residual_segments_file`: the whole list written there as JSON.  A SightJudge that is on leaves its `origin` here: the call is
    then `frame_segment_sight`, and `look`, the sight half of the frame pair just accounted, waits for that judge."""

    def __init__(self, args, world, device, residual):
        self.file = getattr(args, "residual_segments", None)
        self.on = bool(self.file)
        if self.file and not residual.radius:
            raise ValueError("args.residual_segments needs args.residual: the two share the radius")
        if self.file and world > 1:
            raise ValueError("args.residual_segments under more than one rank: merging the lists is not built")
        self.radius, self.device, self.origin, self.look = residual.radius, device, None, None
        self.lists, self.ms, self.judged = {}, [], 0     # frame pair -> its listed segments

    def account(self, number, fp, out):
        with timed(self.device, self.ms):
            if self.origin is not None:
                report, self.look = frame_segment_sight(fp, out, self.device, float(self.radius), self.origin)
            else:
                report = frame_segment_residual(fp, out, self.device, float(self.radius))
        self.judged += sum(1 for v in report.labels.tolist() if v not in utils_eval.RESIDUAL_SKIP_LABELS)
        self.lists[number] = [dict(frame_pair=number, path=fp.name, **e) for e in report.worst(pairs=out["pairs"])]

    def summarise(self, out):
        self.listed = [e for k in sorted(self.lists) for e in self.lists[k]]
        self.listed.sort(key=lambda e: (-e["after_mean"], e["frame_pair"], e["label"]))
        out["residual_segments"] = dict(above=utils_eval.RESIDUAL_EDGES[1], segments_judged=self.judged, segments_listed=len(self.listed),
                                        worst=self.listed[:RESIDUAL_SEGMENTS_SHOWN])
        out["ms_segment_residual_per_frame_pair"] = sum(self.ms) / max(len(self.ms), 1)
        if isinstance(self.file, str):
            with open(self.file, "w") as f:
                json.dump(self.listed, f, indent=1)
            out["residual_segments_file"] = self.file


class SightJudge:
    """args.residual_sight = True or (x, y, z) (`--residual-sight [X Y Z]`; needs args.residual_segments; one process only): the
    line-of-sight check beside the segments' residual -- `frame_segment_sight`, the SegmentJudge's call: per frame pair one depth
    image over the destination as seen from the origin (True: (0, 0, 0)), the codes per segment among the rows further than
    utils_eval.RESIDUAL_EDGES[1] metres from every destination point, one more read-back.  The SegmentResidual is the one the run
    without the attribute gets; every listed segment gains `seen_through`, `excused`, `far_rows` and a `verdict`
    (utils_eval.SegmentSight.annotate), and the summary gains `residual_sight` (params, origin, far, verdicts: listed segments
    per verdict) and `ms_sight_per_frame_pair` (device-synchronised around the image, the table and its read-back only)."""

    def __init__(self, args, world, device, segments):
        sight = getattr(args, "residual_sight", None)
        if sight is not None and sight is not False and not segments.on:
            raise ValueError("args.residual_sight needs args.residual_segments: it judges the segments that one lists")
        self.origin = (0.0, 0.0, 0.0) if sight is True or not sight else tuple(float(v) for v in sight)
        if len(self.origin) != 3:
            raise ValueError(f"args.residual_sight: True or an origin (x, y, z), got {sight!r}")
        self.on = bool(segments.on and sight)
        self.segments, self.device, self.ms = segments, device, []
        if self.on:
            segments.origin = self.origin

    def account(self, number, fp, out):
        with timed(self.device, self.ms, settled=True):
            seen = self.segments.look()
        seen.annotate(self.segments.lists[number])

    def summarise(self, out):
        from . import _lib
        verdicts = {v: sum(1 for e in self.segments.listed if e["verdict"] == v) for v in utils_eval.SIGHT_VERDICTS}
        out["residual_sight"] = dict(params=_lib.SightParams.defaults().as_dict(), origin=list(self.origin), far=utils_eval.RESIDUAL_EDGES[1],
                                     verdicts=verdicts)
        out["ms_sight_per_frame_pair"] = sum(self.ms) / max(len(self.ms), 1)


class TrustJudge:
    """args.residual_trust = True (`--residual-trust`; needs args.residual_segments): one trust byte per source point of every frame
    pair -- `frame_trust` at the shared radius, with the line of sight from the SightJudge's origin iff that judge is on --
    and the summary gains `residual_trust`: the counts added over the frame pairs (utils_eval.TrustCounts.summary, `kept_share`
    among them), `ms_trust_per_frame_pair` (timed on its own, device-synchronised around the chain and its read-back of sixteen
    words) and, where a frame pair carries gt_flow, `epe_kept`, `epe_dropped` and `rows_evaluated`: the mean end-point error of
    the masked rows with and without KEEP, host numpy, their sums added in the order of the frame pairs like every other sum."""

    def __init__(self, args, world, device, segments, sight):
        self.on = bool(getattr(args, "residual_trust", False))
        if self.on and not segments.on:
            raise ValueError("args.residual_trust needs args.residual and args.residual_segments: it spreads their verdicts over the rows")
        self.radius, self.device, self.origin = segments.radius, device, sight.origin if sight.on else None
        self.counts, self.ms, self.epe = utils_eval.TrustCounts(), [], {}    # frame pair -> sum and rows of e: kept, dropped

    def account(self, number, fp, out):
        with timed(self.device, self.ms):
            bytes_, counted = frame_trust(fp, out, self.device, float(self.radius), self.origin)
        self.counts.add(counted)
        if fp.gt_flow is not None:             # (host numpy over the masked rows, like run_stream's meter)
            keep = utils_eval.trust_keep(bytes_).cpu().numpy()
            e = np.linalg.norm(np.asarray(fp.gt_flow, np.float64) - out["flow"].cpu().numpy()[:, 0:3].astype(np.float64), axis=-1)
            judged = np.asarray(fp.mask) > 0 if fp.mask is not None else np.ones(len(e), dtype=bool)
            self.epe[number] = [v for rows_ in (judged & keep, judged & ~keep) for v in (float(e[rows_].sum()), int(rows_.sum()))]

    def summarise(self, out):
        from . import _lib
        block = dict(self.counts.summary(), params=_lib.TrustParams.defaults().as_dict(), line_of_sight=self.origin is not None,
                     ms_trust_per_frame_pair=sum(self.ms) / max(len(self.ms), 1))
        epe = [sum(self.epe[k][at] for k in sorted(self.epe)) for at in range(4)]    # added in the order of the frame pairs
        if epe[1] + epe[3]:
            mean = lambda total, n: total / n if n else float("nan")   # noqa: E731
            block.update(epe_kept=mean(epe[0], epe[1]), epe_dropped=mean(epe[2], epe[3]), rows_evaluated=epe[1] + epe[3])
        out["residual_trust"] = block


class ObjectJudge:
    """args.objects = True or a file name (`--objects [FILE]`; one process only; independent of args.residual): one object row per
    matched pair of every frame pair -- `frame_objects`, outside the timed region of one pair at a time, with
    seconds = fp.gap * args.sweep_seconds (default 0.1) and args.objects_min_speed (default 0.5 m/s).  The summary gains `objects`
    (objects, movers, the pairs without a segment or a box, largest_centre_gap in metres, the parameters) and
    `ms_objects_per_frame_pair` (device-synchronised around the three calls and their one read-back); with a file name, one JSON
    line per frame pair is written there (counts, and per object its labels, centre, size, yaw, velocity, speed, moving,
    centre_gap, point counts) and the summary names it as `objects_file`."""

    def __init__(self, args, world, device):
        self.file = getattr(args, "objects", None)
        self.on = bool(self.file)
        if self.file and world > 1:
            raise ValueError("args.objects under more than one rank: merging the files is not built")
        self.sweep_seconds = float(getattr(args, "sweep_seconds", utils_objects.SWEEP_SECONDS))
        self.min_speed = float(getattr(args, "objects_min_speed", utils_objects.MIN_SPEED))
        self.device = device
        self.lines, self.ms, self.counts, self.gap = {}, [], np.zeros(5, np.int64), None    # frame pair -> its line of the file
        self.parts = {}                            # frame pair -> what it added to the counts, its largest centre gap

    def account(self, number, fp, out):
        with timed(self.device, self.ms):
            seen = frame_objects(fp, out, self.device, float(fp.gap) * self.sweep_seconds, self.min_speed)
        s = seen.summary()
        # (a frame pair accounted a second time -- the TrackJudge's repair of its gap -- replaces what it added the first time)
        self.parts[number] = (np.array([s[name] for name in utils_objects.COUNT_NAMES] + [s["pairs"]], np.int64), seen.largest_centre_gap())
        self.counts = sum((c for c, _ in self.parts.values()), np.zeros(5, np.int64))
        self.gap = max((g for _, g in self.parts.values() if g is not None), default=None)
        self.lines[number] = dict(frame_pair=number, path=fp.name, seconds=seen.seconds, counts=s, objects=seen.as_list())

    def summarise(self, out):
        names = utils_objects.COUNT_NAMES + ("pairs",)
        out["objects"] = dict({name: int(v) for name, v in zip(names, self.counts)}, pairs_without_box=int(self.counts[4] - self.counts[0]),
                              largest_centre_gap=self.gap, sweep_seconds=self.sweep_seconds, min_speed=self.min_speed,
                              delta=utils_objects.BOX_DELTA, directions=utils_objects.BOX_DIRECTIONS)
        out["ms_objects_per_frame_pair"] = sum(self.ms) / max(len(self.ms), 1)
        if isinstance(self.file, str):
            with open(self.file, "w") as f:
                for k in sorted(self.lines):       # one JSON line per frame pair, in their order
                    f.write(json.dumps(self.lines[k]) + "\n")
            out["objects_file"] = self.file


class TrackJudge:
    """args.tracks = True or a file name (`--tracks [FILE]`; one process only; independent of args.objects): the objects of a
    multi-frame sample linked across its gaps -- `frame_tracks` over the frame pairs of one sequence file (they share the
    destination sweep; a frame-pair file is a sample of its own), once the sample's LAST gap has been accounted and in gap order,
    so the tracks do not depend on the order in which frame pairs complete.  It uses the ObjectJudge's args.sweep_seconds and
    args.objects_min_speed and adds args.tracks_min_iou (default 0.5) and args.tracks_max_residual (default 0.2 m).  The summary
    gains `tracks` (samples, tracks, observed, judged, consistent, inconsistent, moving, overflow, the parameters) and
    `ms_tracks_per_sample` (device-synchronised around the chain and its one read-back); with a file name, one JSON line per
    sample is written there (counts, per observed track its velocity, residuals, verdicts and size, and per gap the track of
    every object row) and the summary names it as `tracks_file`.  Where the ObjectJudge keeps lines, every object entry gains
    `track`.  sample_of, samples: the maps that frame_pairs._by_sample fills as the frame pairs go by.

    args.tracks_repair = True (`--tracks-repair`; needs args.tracks): `frame_tracks(repair=True)` -- a gap that alone breaks its
    track is registered again and, where accepted, the `out` of that frame pair carries the new transform, pair row and flow from
    then on; the ObjectJudge accounts such a frame pair again (its line and its counts are replaced).  A sample's line gains
    `repair` (per retried pair its gap, frame pair, pair row, labels, track, reason, e_old, e_new, distance from the prediction,
    accepted), the summary `tracks_repair` (suspects, retried, accepted, a count per reason, consistent_before / consistent_after)
    and `ms_tracks_repair_per_sample` (behind the tracks' first read-back, to the end of the second chain).  What run_stream
    scored of a frame pair's flow at its delivery (files with ground truth) is of the registration as delivered.

    args.tracks_fill = True (`--tracks-fill`; needs args.tracks): `frame_tracks(fill=True)`, after the repair when both are set -- a
    gap in which a track found no pair is registered from what the other gaps predict and, where accepted, the `out` of that
    frame pair carries one more pair row and transform and the flow of that cluster from then on; the ObjectJudge accounts such a
    frame pair again.  A sample's line gains `fill` (per missing (track, gap) its gap, frame pair, destination segment, track,
    labels, reason, and where it was registered e_old, e_new, distance from the prediction, accepted, the appended pair row), the
    summary `tracks_fill` (missing, retried, accepted, a count per reason, observed_before / observed_after, judged_before /
    judged_after) and `ms_tracks_fill_per_sample` (behind the tracks' read-back, to the end of the last chain)."""

    def __init__(self, args, world, device, objects, sample_of, samples):
        self.file = getattr(args, "tracks", None)
        self.on = bool(self.file)
        if self.file and world > 1:
            raise ValueError("args.tracks under more than one rank: a sample's gaps would have to meet on one rank, which is not built")
        self.min_iou = float(getattr(args, "tracks_min_iou", utils_tracks.MIN_IOU))
        self.max_residual = float(getattr(args, "tracks_max_residual", utils_tracks.MAX_RESIDUAL))
        self.device, self.objects, self.sample_of, self.samples = device, objects, sample_of, samples
        self.lines, self.ms = {}, []               # sample -> its line of the file
        self.totals = dict(tracks=0, observed=0, judged=0, consistent=0, inconsistent=0, moving=0, overflow=0)
        self.repair, self.args = bool(getattr(args, "tracks_repair", False)), args
        if self.repair and not self.on:
            raise ValueError("args.tracks_repair goes with args.tracks (it registers again what the tracks name)")
        self.ms_repair = []
        self.fill = bool(getattr(args, "tracks_fill", False))
        if self.fill and not self.on:
            raise ValueError("args.tracks_fill goes with args.tracks (it fills the gaps the tracks name)")
        self.ms_fill = []
        self.filled = dict(missing=0, retried=0, accepted=0, reasons={name: 0 for name in utils_tracks.FILL_REASONS}, observed_before=0, observed_after=0,
                           judged_before=0, judged_after=0)
        self.repaired = dict(suspects=0, retried=0, accepted=0, reasons={name: 0 for name in utils_tracks.REPAIR_REASONS}, consistent_before=0,
                             consistent_after=0)

    def account(self, number, fp, out):
        sample = self.samples[self.sample_of.pop(number)]
        sample["outs"][number] = (fp, out)
        if len(sample["outs"]) < sample["size"]:
            return
        # the chain of the sample, once every gap of it has been accounted: in gap order, whatever order they completed in
        s = sample["sample"]
        del self.samples[s]
        ks = sorted(sample["outs"])
        fps = [sample["outs"][k][0] for k in ks]
        with timed(self.device, self.ms):
            seen = frame_tracks(fps, [sample["outs"][k][1] for k in ks], self.device, self.objects.sweep_seconds, self.objects.min_speed,
                                self.min_iou, self.max_residual, repair=self.repair, args=self.args, **(dict(fill=True) if self.fill else {}))
        summary = seen.summary()
        for name in self.totals:
            self.totals[name] += summary[name]
        self.lines[s] = dict(sample=s, path=fps[0].sequence or fps[0].name, frame_pairs=ks, gaps=[fp.gap for fp in fps], counts=summary,
                             tracks=seen.as_list(), observations=[ids.tolist() for ids in seen.observation_ids])
        if self.repair:
            done = seen.repair.summary(seen.fill.before if self.fill else seen)       # (the repair's block is what it is alone)
            for name, v in done.items():
                if name == "reasons":
                    for reason, c in v.items():
                        self.repaired["reasons"][reason] += c
                else:
                    self.repaired[name] += v
            self.ms_repair.append(seen.repair.ms)
            self.lines[s]["repair"] = [dict(e, frame_pair=ks[e["gap"]], reason=utils_tracks.REPAIR_REASONS[e["reason"]]) for e in seen.repair.retried]
            if self.objects.on:                     # the objects of a repaired gap, again: its line and its counts are replaced
                for g in sorted({e["gap"] for e in seen.repair.retried if e["accepted"]}):
                    self.objects.account(ks[g], fps[g], sample["outs"][ks[g]][1])
        if self.fill:
            done = seen.fill.summary(seen)
            for name, v in done.items():
                if name == "reasons":
                    for reason, c in v.items():
                        self.filled["reasons"][reason] += c
                else:
                    self.filled[name] += v
            self.ms_fill.append(seen.fill.ms)
            self.lines[s]["fill"] = [dict(e, frame_pair=ks[e["gap"]], reason=utils_tracks.FILL_REASONS[e["reason"]]) for e in seen.fill.retried]
            if self.objects.on:                     # the objects of a filled gap, again: its line and its counts are replaced
                for g in sorted({e["gap"] for e in seen.fill.retried if e["accepted"]}):
                    self.objects.account(ks[g], fps[g], sample["outs"][ks[g]][1])
        for k, ids in zip(ks, seen.observation_ids):
            for e in self.objects.lines.get(k, {}).get("objects", []):
                e["track"] = int(ids[e["pair"]])

    def summarise(self, out):
        out["tracks"] = dict(self.totals, samples=len(self.lines), min_iou=self.min_iou, max_residual=self.max_residual,
                             min_speed=self.objects.min_speed, sweep_seconds=self.objects.sweep_seconds)
        out["ms_tracks_per_sample"] = sum(self.ms) / max(len(self.ms), 1)
        if self.repair:
            out["tracks_repair"] = dict(self.repaired)
            out["ms_tracks_repair_per_sample"] = sum(self.ms_repair) / max(len(self.ms_repair), 1)
        if self.fill:
            out["tracks_fill"] = dict(self.filled)
            out["ms_tracks_fill_per_sample"] = sum(self.ms_fill) / max(len(self.ms_fill), 1)
        if isinstance(self.file, str):
            with open(self.file, "w") as f:
                for s in sorted(self.lines):        # one JSON line per sample, in their order
                    f.write(json.dumps(self.lines[s]) + "\n")
            out["tracks_file"] = self.file


class LogTrackJudge:
    """args.tracks_log = True or a file name (`--tracks-log [FILE]`; one process only; independent of args.tracks and
    args.objects): the objects of a LOG linked from file to file -- the frame pairs of the stream are consecutive files, file k
    registers sweep k onto sweep k + 1 -- by `LogChain`: the files are added in the stream's order whatever order they complete
    in (a file that completes early waits for the ones before it), and `close`, once the stream is through, reads the whole log
    back at once.  It uses the ObjectJudge's args.sweep_seconds and args.objects_min_speed and adds args.tracks_log_radius
    (default 0.02 m), args.tracks_log_min_share (default 0.5) and args.tracks_log_max_dv (default 1.0 m/s).  The summary gains
    `tracks_log` (files, tracks, observed, judged, smooth, rough, moving, breaks, carried_rows, rows, overflow, the parameters)
    and `ms_tracks_log_per_file` (device-synchronised around every file's chain and around the closing call with its read-back);
    with a file name, one JSON line per track is written there (its table row, and per object row of the track its step, file,
    pair and velocity in the log's frame) and the summary names it as `tracks_log_file`.  Where the ObjectJudge keeps lines,
    every object entry gains `log_track`.  A frame pair of a multi-frame sample is refused: which sweeps consecutive samples
    share is not in their files."""

    def __init__(self, args, world, device, objects):
        self.file = getattr(args, "tracks_log", None)
        self.on = bool(self.file)
        if self.file and world > 1:
            raise ValueError("args.tracks_log under more than one rank: a log's files would have to meet on one rank in their order, which is not built")
        self.device, self.objects = device, objects
        self.waiting, self.next, self.ms, self.numbers = {}, 0, [], []
        self.chain = None
        if self.on:
            self.chain = LogChain(device, objects.sweep_seconds, objects.min_speed, float(getattr(args, "tracks_min_iou", utils_tracks.MIN_IOU)),
                                  float(getattr(args, "tracks_log_radius", utils_tracks.CARRY_RADIUS)),
                                  float(getattr(args, "tracks_log_min_share", utils_tracks.CARRY_MIN_SHARE)),
                                  float(getattr(args, "tracks_log_max_dv", utils_tracks.MAX_DV)))

    def account(self, number, fp, out):
        if fp.sequence is not None:
            raise ValueError(f"args.tracks_log: {fp.name!r} is a gap of a multi-frame sample; a log is a stream of frame-pair files "
                             "(utils_tracks.TrackState(track_of_row=...) composes logs of samples)")
        self.waiting[number] = (fp, out)
        while self.next in self.waiting:          # in the stream's order, whatever order the frame pairs completed in
            fp, out = self.waiting.pop(self.next)
            with timed(self.device, self.ms):
                self.chain.add(fp, out)
            self.numbers.append(self.next)
            self.next += 1

    def close(self):
        """after the stream's last frame pair: the table over the log, the one read-back, the ids into the ObjectJudge's lines"""
        if self.waiting:
            raise RuntimeError(f"args.tracks_log: frame pairs {sorted(self.waiting)} arrived, {self.next} never did")
        with timed(self.device, self.ms):
            self.seen = self.chain.read()
        for k, ids in zip(self.numbers, self.seen.observation_ids):
            for e in self.objects.lines.get(k, {}).get("objects", []):
                e["log_track"] = int(ids[e["pair"]])

    def summarise(self, out):
        out["tracks_log"] = dict(self.seen.summary(), **self.seen.params)
        out["ms_tracks_log_per_file"] = sum(self.ms) / max(len(self.numbers), 1)
        if isinstance(self.file, str):
            with open(self.file, "w") as f:
                for e in self.seen.as_list():       # one JSON line per track, in the order of the ids
                    f.write(json.dumps(e) + "\n")
            out["tracks_log_file"] = self.file

"""Object tracks: the clusters of a sample's shared destination sweep linked across its gaps, and one constant velocity per
track (include/icpflow_hip.h, "8(k) object tracks"; csrc/overlap.hip, csrc/tracks.hip).  No counterpart in the reference.

Every frame pair of a multi-frame sample ends at frame 0, and every gap clusters that sweep anew.  Two labellings of the same
rows say which clusters are the same object (`label_overlap_device`); `TrackState.extend` carries one id per object from gap
to gap and turns the gap's object rows (utils_objects) into observations; `TrackState.fit` fits d = s v per track over all
gaps.  min_iou, max_residual and min_speed are stated policies, like KEEP of the trust byte.

Across the files of a LOG (8(l); csrc/carry.hip) the shared sweep is the destination of one file and the source of the next, in
another frame and with other rows: `rows_carry_device` carries the ids by nearest rows under the file's pose, a `TrackState`
seeded with them links the file's SOURCE clusters (`extend(side=0)`), `pair_row_ids_device` hands the ids to the destination
rows for the next file, and `LogTracks` is the table over the log (pair_judges.LogChain runs the chain).  The radius, min_share
and max_dv are stated policies too.

Everything stays on the device until `TrackState.read` (`LogChain.read`) reads it back, once.  There is no CPU path."""
import ctypes

import numpy as np

MIN_IOU = 0.5
MAX_RESIDUAL = 0.2            # metres
MIN_SPEED = 0.5               # m/s (utils_objects.MIN_SPEED)
MAX_ID = 1 << 24
CARRY_RADIUS = 0.02           # metres: far above the float32 rounding of a pose product at 100 m (8e-6 m), below the spacing at
                              # which a wrong neighbour would belong to another cluster -- a stated policy
CARRY_MIN_SHARE = 0.5         # fewer rows of a view with a partner in the other: the chain of ids breaks and starts afresh
MAX_DV = 1.0                  # m/s between adjacent steps: 10 cm per 0.1 s sweep


def label_overlap_device(labels_a, labels_b, Lmax=4096):
    """icpflow_label_overlap enqueued on the current stream, nothing read back.  labels_a, labels_b [n]: two labellings of the
    same rows, device tensors.  -> (table_a float64 [Lmax, 10], num_a int32 [1], table_b, num_b, counts int64 [4]) on the device;
    rows of a table from its number on are not written, and neither table is when a number is negative."""
    import torch
    from . import _lib
    _lib.require_gpu(labels_a, labels_b)
    a, b = labels_a.to(torch.float32).contiguous(), labels_b.to(torch.float32).contiguous()
    n, device, Lmax = int(a.shape[0]), a.device, int(Lmax)
    if a.dim() != 1 or b.shape != a.shape or b.device != device:
        raise ValueError(f"label_overlap: labels {tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}, expected two of [n] on one device")
    tables = [torch.empty((Lmax, _lib.OVERLAP_COLS), dtype=torch.float64, device=device) for _ in range(2)]
    nums = [torch.empty(1, dtype=torch.int32, device=device) for _ in range(2)]
    counts = torch.empty(_lib.OVERLAP_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        ws = _lib.workspace(device, int(_lib._L.icpflow_label_overlap_workspace_bytes(n, Lmax)))
        _lib.call("icpflow_label_overlap", _lib.ptr(a), _lib.ptr(b), n, Lmax, _lib.ptr(tables[0]), _lib.ptr(nums[0]), _lib.ptr(tables[1]),
                  _lib.ptr(nums[1]), _lib.ptr(counts), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return tables[0], nums[0], tables[1], nums[1], counts


def rows_carry_device(prev, prev_id, pose, nxt, radius=CARRY_RADIUS, min_share=CARRY_MIN_SHARE):
    """icpflow_rows_carry enqueued on the current stream, nothing read back.  prev float32 [m, 3] and prev_id int32 [m]: one view
    of a sweep and an id per row (device tensors); pose: a 4 x 4 on the HOST that maps prev's coordinates into nxt's; nxt
    float32 [n, 3]: the other view.  -> (ids int32 [n], counts int64 [6]) on the device: the id of the nearest moved row within
    `radius`, all -1 when fewer than min_share * n rows found one (counts[5])."""
    import torch
    from . import _lib
    _lib.require_gpu(prev, prev_id, nxt)
    a, b = prev.to(torch.float32).contiguous(), nxt.to(torch.float32).contiguous()
    ids = prev_id.to(torch.int32).contiguous()
    m, n, device = int(a.shape[0]), int(b.shape[0]), b.device
    if tuple(a.shape) != (m, 3) or tuple(b.shape) != (n, 3) or tuple(ids.shape) != (m,) or a.device != device or ids.device != device:
        raise ValueError(f"rows_carry: views {tuple(a.shape)} and {tuple(b.shape)}, ids {tuple(ids.shape)}: expected [m, 3], [n, 3] and [m] on one device")
    h_pose = np.ascontiguousarray(np.asarray(pose, np.float64).reshape(16))
    out = torch.empty(n, dtype=torch.int32, device=device)
    counts = torch.empty(_lib.CARRY_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        ws = _lib.workspace(device, int(_lib._L.icpflow_rows_carry_workspace_bytes(n, m)))
        _lib.call("icpflow_rows_carry", _lib.ptr(a) if m else None, _lib.ptr(ids) if m else None, m, h_pose.ctypes.data_as(ctypes.c_void_p),
                  _lib.ptr(b) if n else None, n, float(radius), float(min_share), _lib.ptr(out) if n else None, None, None, _lib.ptr(counts),
                  _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return out, counts


def pair_row_ids_device(labels, pair_rows, col, pair_id, weight=None):
    """icpflow_pair_row_ids enqueued on the current stream.  labels [n] of one side of a frame pair, pair_rows float32 [P, >= 2]
    (column 0 the source label, column 1 the destination label), col 0 or 1: that side; pair_id int32 [P]; weight: a float64
    COLUMN of P values (a strided view such as objects_rows[:, 22] is taken as it is), or None.  -> (ids int32 [n], counts
    int64 [3]) on the device."""
    import torch
    from . import _lib
    _lib.require_gpu(labels, pair_rows, pair_id, weight)
    lab = labels.to(torch.float32).contiguous()
    n, device = int(lab.shape[0]), lab.device
    P = 0 if pair_rows is None else int(pair_rows.shape[0])
    rows = pid = None
    stride, wstride = 2, 1
    if P > 0:
        rows, pid = pair_rows.to(torch.float32).contiguous(), pair_id.to(torch.int32).contiguous()
        stride = int(rows.shape[1])
        if rows.dim() != 2 or stride < 2 or tuple(pid.shape) != (P,) or rows.device != device or pid.device != device:
            raise ValueError(f"pair_row_ids: pair rows {tuple(rows.shape)}, ids {tuple(pid.shape)}: expected [P, >= 2] and [P] on the labels' device")
        if weight is not None:
            if weight.dtype != torch.float64 or tuple(weight.shape) != (P,) or weight.device != device or (P > 1 and weight.stride(0) < 1):
                raise ValueError(f"pair_row_ids: weights {tuple(weight.shape)} {weight.dtype}, expected float64 [P] on the labels' device")
            wstride = int(weight.stride(0)) if P > 1 else 1
    out = torch.empty(n, dtype=torch.int32, device=device)
    counts = torch.empty(_lib.PAIR_ROW_ID_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        ws = _lib.workspace(device, int(_lib._L.icpflow_pair_row_ids_workspace_bytes(P)))
        _lib.call("icpflow_pair_row_ids", _lib.ptr(lab) if n else None, n, _lib.ptr(rows), P, stride, int(col), _lib.ptr(pid),
                  ctypes.c_void_p(weight.data_ptr()) if (P > 0 and weight is not None) else None, wstride, _lib.ptr(out) if n else None,
                  _lib.ptr(counts), _lib.ptr(ws), ctypes.c_size_t(ws.numel()), _lib.stream(device))
    return out, counts


class TrackState:
    """The tracks of ONE shared sweep of n rows, on the device: a track id per row and the next free id, carried from gap to gap
    by `extend`; `fit` and `read` close the sample.  track_of_row int32 [n] and next_id int32 [1] (device tensors, taken BY
    REFERENCE and written by `extend`) seed the state with ids carried over from elsewhere (`rows_carry_device`) and a running
    id counter, for tracks that outlive a sample; `bound`: an upper bound of that counter on entry."""

    def __init__(self, n, device, Lmax=4096, min_iou=MIN_IOU, max_residual=MAX_RESIDUAL, min_speed=MIN_SPEED, track_of_row=None, next_id=None,
                 bound=0):
        import torch
        from . import _lib
        self.n, self.device, self.Lmax = int(n), torch.device(device), int(Lmax)
        if self.device.type != "cuda":
            raise RuntimeError("icp_flow_amd: the tracks live on a GPU (HIP) device -- there is no CPU path")
        self.params = _lib.TrackParams.defaults(min_iou=min_iou, max_residual=max_residual, min_speed=min_speed)
        for name, t, shape in (("track_of_row", track_of_row, (self.n,)), ("next_id", next_id, (1,))):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"TrackState: {name} {tuple(t.shape)} {t.dtype} on {t.device}, expected contiguous int32 {list(shape)} on {self.device}")
        self.track_of_row = torch.full((self.n,), -1, dtype=torch.int32, device=self.device) if track_of_row is None else track_of_row
        self.next_id = torch.zeros(1, dtype=torch.int32, device=self.device) if next_id is None else next_id
        self.obs, self.gaps, self.segments, self.counts = [], [], [], []
        self.bound = int(bound)              # no track id reaches this: every gap founds at most min(n, Lmax) tracks
        self.tracks = self.fit_counts = None

    def extend(self, labels, objects_rows, gap, seconds, side=1):
        """One gap: labels [n] of the shared sweep under this gap's clustering, objects_rows float64 [P, 24] (or None) the gap's
        table of utils_objects.pair_objects_device.  side 1: the sweep is the pairs' destination (a sample's gaps); side 0: it is
        their source (the files of a log).  Enqueued on the current stream.  -> (segments float64 [Lmax, 6], num int32
        [1], obs float64 [P, 13], counts int64 [6]) on the device, kept for `read` as well."""
        import torch
        from . import _lib
        _lib.require_gpu(labels, objects_rows)
        lab = labels.to(torch.float32).contiguous()
        if lab.shape != (self.n,) or lab.device != self.device:
            raise ValueError(f"TrackState.extend: labels {tuple(lab.shape)} on {lab.device} for a sweep of {self.n} rows on {self.device}")
        rows = None
        P = 0 if objects_rows is None else int(objects_rows.shape[0])
        if P > 0:
            rows = objects_rows.contiguous()
            if rows.dtype != torch.float64 or tuple(rows.shape) != (P, _lib.OBJECT_COLS) or rows.device != self.device:
                raise ValueError(f"TrackState.extend: object rows {tuple(rows.shape)} {rows.dtype}, expected float64 [P, {_lib.OBJECT_COLS}]")
        segments = torch.empty((self.Lmax, _lib.TRACK_SEGMENT_COLS), dtype=torch.float64, device=self.device)
        num = torch.empty(1, dtype=torch.int32, device=self.device)
        obs = torch.empty((P, _lib.TRACK_OBS_COLS), dtype=torch.float64, device=self.device)
        counts = torch.empty(_lib.TRACK_EXTEND_COUNTS, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            ws = _lib.workspace(self.device, int(_lib._L.icpflow_object_tracks_extend_workspace_bytes(self.n, self.Lmax)))
            _lib.call("icpflow_object_tracks_extend_side", _lib.ptr(lab) if self.n else None, self.n, self.Lmax,
                      _lib.ptr(self.track_of_row) if self.n else None, _lib.ptr(self.next_id), _lib.ptr(rows), P, int(side), int(gap), float(seconds),
                      ctypes.byref(self.params), _lib.ptr(segments), _lib.ptr(num), _lib.ptr(obs) if P else None, _lib.ptr(counts), _lib.ptr(ws),
                      ctypes.c_size_t(ws.numel()), _lib.stream(self.device))
        self.obs.append(obs), self.gaps.append(int(gap)), self.segments.append((segments, num)), self.counts.append(counts)
        self.bound = min(self.bound + min(self.n, self.Lmax), MAX_ID)
        self.tracks = None
        return segments, num, obs, counts

    def fit(self):
        """icpflow_object_tracks_fit over the observations of every gap so far, enqueued on the current stream.  The number of
        tracks is on the device; the call takes the bound the gaps imply (a track beyond *next_id has its id and zeros).
        -> (tracks float64 [bound, 16], counts int64 [5]) on the device."""
        import torch
        from . import _lib
        every = torch.cat(self.obs) if self.obs else torch.empty((0, _lib.TRACK_OBS_COLS), dtype=torch.float64, device=self.device)
        M, T = int(every.shape[0]), self.bound
        self.tracks = torch.empty((T, _lib.TRACK_COLS), dtype=torch.float64, device=self.device)
        self.fit_counts = torch.empty(_lib.TRACK_FIT_COUNTS, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("icpflow_object_tracks_fit", _lib.ptr(every) if M else None, M, T, ctypes.byref(self.params), _lib.ptr(self.tracks) if T else None,
                      _lib.ptr(self.fit_counts), _lib.stream(self.device))
        return self.tracks, self.fit_counts

    def read(self):
        """-> Tracks: the fitted table, the counts of every call and the observations' ids in ONE transfer (ids and counts are
        exact in a float64)"""
        import torch
        if self.tracks is None:
            self.fit()
        f64 = lambda t: t.to(torch.float64).reshape(-1)     # noqa: E731
        parts = [f64(self.next_id), f64(self.fit_counts)] + [f64(c) for c in self.counts] + [o[:, 0].reshape(-1) for o in self.obs] + [self.tracks.reshape(-1)]
        host = torch.cat(parts).cpu().numpy()
        at = 0

        def take(k):
            nonlocal at
            at += k
            return host[at - k: at]

        next_id = int(take(1)[0])
        fit_counts = np.rint(take(5)).astype(np.int64)
        extend_counts = [np.rint(take(6)).astype(np.int64) for _ in self.counts]
        ids = [np.rint(take(int(o.shape[0]))).astype(np.int64) for o in self.obs]
        rows = take(self.bound * 16).reshape(self.bound, 16)[:next_id]
        return Tracks(rows, fit_counts, next_id, list(self.gaps), ids, extend_counts, self.params.as_dict())


REPAIR_REASONS = ("accepted", "reject_test", "error", "off_prediction", "not_better", "abandoned", "too_long")
REPAIR_TOO_LONG = 6            # a cluster longer than args.max_points: not retried (its subsample would draw random numbers)


def suspects_device(obs, T, max_residual=MAX_RESIDUAL):
    """icpflow_object_tracks_suspects enqueued on the current stream, nothing read back.  obs float64 [M, 13]: the observations of
    every gap, concatenated as `TrackState.fit` concatenates them; T: the tracks (an upper bound).  -> (plan float64 [M, 8],
    counts int64 [4]) on the device: per observation whether it alone breaks its track, and the displacement the others predict."""
    import torch
    from . import _lib
    _lib.require_gpu(obs)
    M, device = int(obs.shape[0]), obs.device
    if obs.dtype != torch.float64 or tuple(obs.shape) != (M, _lib.TRACK_OBS_COLS):
        raise ValueError(f"suspects: observations {tuple(obs.shape)} {obs.dtype}, expected float64 [M, {_lib.TRACK_OBS_COLS}]")
    rows = obs.contiguous()
    plan = torch.empty((M, _lib.TRACK_PLAN_COLS), dtype=torch.float64, device=device)
    counts = torch.empty(_lib.TRACK_PLAN_COUNTS, dtype=torch.int64, device=device)
    params = _lib.TrackParams.defaults(max_residual=max_residual)
    with torch.cuda.device(device):
        _lib.call("icpflow_object_tracks_suspects", _lib.ptr(rows) if M else None, M, int(T), ctypes.byref(params), _lib.ptr(plan) if M else None,
                  _lib.ptr(counts), _lib.stream(device))
    return plan, counts


def repair_params(args, translation_frame, max_residual=MAX_RESIDUAL):
    """_lib.RepairParams of the association's thresholds in `args` (thres_iou, thres_rot * 90 degrees, thres_error), the gap's
    translation_frame and the tracks' max_residual"""
    from . import _lib
    return _lib.RepairParams.defaults(translation_frame=float(translation_frame), thres_iou=float(args.thres_iou), rot_limit_deg=float(args.thres_rot) * 90.0,
                                      thres_error=float(args.thres_error), max_residual=float(max_residual))


def reregister_device(args, st, dt, si, di, T_old, centre, pred, params):
    """icpflow_pairs_reregister enqueued on the current stream, nothing read back: K pairs of ONE frame pair registered again
    from the pure translations [I | pred].  st, dt: the gap's utils_check.ClusterTable of the ego-compensated source and of the
    destination (fetched); si, di: the K pairs' rows of the two tables (numpy), none of them longer than args.max_points -- the
    repair draws no random numbers; T_old float32 [K, 4, 4], centre and pred float64 [K, 3]: device tensors; params: a
    _lib.RepairParams.  -> dict(T float32 [K, 4, 4], report float64 [K, 12], counts int64 [8], T_new, errors, inliers, ratios,
    ious [K, 2], iterations int32 [1]) on the device; the metrics are the new poses', views of the call's workspace."""
    import torch
    from . import _lib, utils_match
    _lib.require_gpu(T_old, centre, pred)
    device, K = st.points.device, len(si)
    if K < 1 or len(di) != K or int(max(st.h_count[si].max(), dt.h_count[di].max())) > int(args.max_points):
        raise ValueError(f"reregister: {K} source and {len(di)} destination clusters, the longest beyond max_points = {args.max_points}?")
    old = T_old.to(device=device, dtype=torch.float32).reshape(K, 16).contiguous()
    c, p = (t.to(device=device, dtype=torch.float64).reshape(K, 3).contiguous() for t in (centre, pred))
    init = torch.eye(4, dtype=torch.float32, device=device).repeat(K, 1, 1)
    init[:, 0:3, 3] = p.to(torch.float32)
    key, base, _, N, has_perm = utils_match._stage_rows(args, st, dt, si, di)
    assert not has_perm
    max_it, rel, stop = utils_match._icp_options(args)
    reg = _lib.Registration(None, None, None, 0, 0, 0, 0.0, float(args.thres_dist), float(rel), int(max_it), int(stop))
    tables = _lib.Tables(st.points.data_ptr(), st.order.data_ptr(), st._packed.data_ptr() + 8, dt.points.data_ptr(), dt.order.data_ptr(),
                         dt._packed.data_ptr() + 8, len(st.h_labels), len(dt.h_labels), 9)
    clouds = torch.empty((2, K, N, 4), dtype=torch.float32, device=device)
    T = torch.empty((K, 16), dtype=torch.float32, device=device)
    report = torch.empty((K, _lib.REPAIR_COLS), dtype=torch.float64, device=device)
    counts = torch.empty(_lib.REPAIR_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        need = int(_lib._L.icpflow_pairs_reregister_workspace_bytes(K, N))
        ws = torch.empty(need, dtype=torch.uint8, device=device)        # (its first region is handed back: not the cached scratch)
        _lib.call("icpflow_pairs_reregister", ctypes.byref(tables), K, N, ctypes.c_void_p(base), _lib.ptr(clouds), _lib.ptr(init), _lib.ptr(old),
                  _lib.ptr(c), _lib.ptr(p), ctypes.byref(reg), ctypes.byref(params), _lib.ptr(T), _lib.ptr(report), _lib.ptr(counts), _lib.ptr(ws),
                  ctypes.c_size_t(need), _lib.stream(device), _lib.opt())
    utils_match._Staging.done(key)
    words = ws[: 4 * (44 * K + 1)].view(torch.float32)
    part = lambda a, b, cols: words[a * K: b * K].view(K, cols)    # noqa: E731
    return dict(T=T.view(K, 4, 4), report=report, counts=counts, T_new=part(0, 16, 16).view(K, 4, 4), errors=part(16, 18, 2), inliers=part(18, 20, 2),
                ratios=part(20, 22, 2), ious=part(22, 24, 2), iterations=words[44 * K:].view(torch.int32), keep=(ws, clouds, init, old, c, p))


class Repair:
    """What frame_tracks(repair=True) did to one sample, on the host: `before` the Tracks as the registrations left them,
    `plan_counts` icpflow_object_tracks_suspects' four counts, `retried` one dict per suspect pair (gap: its index among the
    sample's frame pairs, pair: its row of that gap's tables, labels, track, reason, e_old, e_new, distance: of the new
    displacement from the predicted one in xy, accepted), `counts` the eight words (reasons 0 to 5 by the device, 6 by the host)."""

    def __init__(self, before, plan_counts, retried, counts, ms=0.0):
        self.before, self.retried, self.ms = before, list(retried), float(ms)     # ms: the repair's wall time behind the first read-back
        self.plan_counts, self.counts = np.asarray(plan_counts, np.int64).reshape(4), np.asarray(counts, np.int64).reshape(8)

    def summary(self, after):
        return dict(suspects=int(self.plan_counts[3]), retried=int(self.counts[:6].sum()), accepted=int(self.counts[0]),
                    reasons={name: int(v) for name, v in zip(REPAIR_REASONS, self.counts)},
                    consistent_before=int(self.before.fit_counts[3]), consistent_after=int(after.fit_counts[3]))


FILL_RADIUS = 1.0              # metres: below the centre distance of two parked cars side by side, above the wander of a box centre
                               # between two views of one object -- a stated policy
FILL_REASONS = REPAIR_REASONS + ("no_candidate", "lost")
FILL_NO_CANDIDATE, FILL_LOST = 7, 8


def missing_device(obs, T, segments, nums, gaps, seconds, max_residual=MAX_RESIDUAL):
    """icpflow_object_tracks_missing enqueued on the current stream, nothing read back.  obs float64 [M, 13]: the observations of
    every gap, concatenated; T: the tracks (an upper bound); segments float64 [G, Lmax, 6] and nums int32 [G]: what
    `TrackState.extend` left per gap slot, stacked; gaps, seconds: per slot (HOST) the gap its observations carry and the seconds
    it spans.  -> (plan float64 [G, Lmax, 14], counts int64 [G, 4]) on the device: per segment of every slot whether its track
    lacks a pair there, and what the other gaps predict (p: the displacement, q: the source box's centre).  The plan is allocated
    as zeros: the rows the call does not write read as not missing."""
    import torch
    from . import _lib
    _lib.require_gpu(obs, segments, nums)
    M, device = int(obs.shape[0]), segments.device
    G, Lmax = (int(v) for v in segments.shape[:2]) if segments.dim() == 3 else (0, 0)
    if obs.dtype != torch.float64 or tuple(obs.shape) != (M, _lib.TRACK_OBS_COLS) or obs.device != device:
        raise ValueError(f"missing: observations {tuple(obs.shape)} {obs.dtype}, expected float64 [M, {_lib.TRACK_OBS_COLS}]")
    if segments.dtype != torch.float64 or tuple(segments.shape) != (G, Lmax, _lib.TRACK_SEGMENT_COLS) or nums.dtype != torch.int32 or tuple(nums.shape) != (G,):
        raise ValueError(f"missing: segments {tuple(segments.shape)} {segments.dtype}, numbers {tuple(nums.shape)} {nums.dtype}: expected float64 "
                         f"[G, Lmax, {_lib.TRACK_SEGMENT_COLS}] and int32 [G]")
    h_gap = np.ascontiguousarray(np.asarray(gaps, np.int32).reshape(-1))
    h_seconds = np.ascontiguousarray(np.asarray(seconds, np.float64).reshape(-1))
    if len(h_gap) != G or len(h_seconds) != G:
        raise ValueError(f"missing: {len(h_gap)} gaps and {len(h_seconds)} seconds for {G} slots")
    rows, seg, num = obs.contiguous(), segments.contiguous(), nums.contiguous()
    plan = torch.zeros((G, Lmax, _lib.TRACK_MISSING_COLS), dtype=torch.float64, device=device)
    counts = torch.empty((G, _lib.TRACK_MISSING_COUNTS), dtype=torch.int64, device=device)
    params = _lib.TrackParams.defaults(max_residual=max_residual)
    with torch.cuda.device(device):
        _lib.call("icpflow_object_tracks_missing", _lib.ptr(rows) if M else None, M, int(T), _lib.ptr(seg), _lib.ptr(num), G, Lmax,
                  h_gap.ctypes.data_as(ctypes.c_void_p), h_seconds.ctypes.data_as(ctypes.c_void_p), ctypes.byref(params), _lib.ptr(plan),
                  _lib.ptr(counts), _lib.stream(device))
    return plan, counts


def fill_candidates_device(q, boxes_src, num_src, pair_rows, radius=FILL_RADIUS, max_rows=10000):
    """icpflow_pairs_fill_candidates enqueued on the current stream, nothing read back.  q float64 [K, 3]: the predicted source
    box centres of ONE gap's missing rows; boxes_src float64 [Lmax, 16], num_src int32 [1]: utils_objects.segment_boxes_device's
    table of that gap's ego-compensated source; pair_rows float32 [P, >= 1] (or None): column 0 the source labels already
    matched.  -> (choice float64 [K, 8], counts int64 [4]) on the device: per row the nearest unmatched box within `radius`."""
    import torch
    from . import _lib
    _lib.require_gpu(q, boxes_src, num_src, pair_rows)
    K, device, Lmax = int(q.shape[0]), boxes_src.device, int(boxes_src.shape[0])
    if q.dtype != torch.float64 or tuple(q.shape) != (K, 3) or q.device != device:
        raise ValueError(f"fill_candidates: q {tuple(q.shape)} {q.dtype}, expected float64 [K, 3] on the boxes' device")
    if boxes_src.dtype != torch.float64 or tuple(boxes_src.shape) != (Lmax, _lib.BOX_COLS) or num_src.dtype != torch.int32:
        raise ValueError(f"fill_candidates: boxes {tuple(boxes_src.shape)} {boxes_src.dtype}, expected float64 [Lmax, {_lib.BOX_COLS}] and an int32 number")
    P = 0 if pair_rows is None else int(pair_rows.shape[0])
    rows, stride = None, 1
    if P > 0:
        rows = pair_rows.to(device=device, dtype=torch.float32).contiguous()
        if rows.dim() != 2 or rows.shape[1] < 1:
            raise ValueError(f"fill_candidates: pair rows {tuple(rows.shape)}, expected [P, >= 1]")
        stride = int(rows.shape[1])
    centres, boxes, num = q.contiguous(), boxes_src.contiguous(), num_src.contiguous()
    choice = torch.empty((K, _lib.FILL_CHOICE_COLS), dtype=torch.float64, device=device)
    counts = torch.empty(_lib.FILL_COUNTS, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _lib.call("icpflow_pairs_fill_candidates", _lib.ptr(centres) if K else None, K, _lib.ptr(boxes), _lib.ptr(num), Lmax, _lib.ptr(rows), P, stride,
                  float(radius), int(max_rows), _lib.ptr(choice) if K else None, _lib.ptr(counts), _lib.stream(device))
    return choice, counts


class Fill:
    """What frame_tracks(fill=True) did to one sample, on the host: `before` the Tracks as the registrations (and the repair) left
    them, `plan_counts` icpflow_object_tracks_missing's four counts added over the gap slots, `retried` one dict per missing
    (track, gap) (gap: its index among the sample's frame pairs, segment: the destination segment of that gap's labelling,
    track, labels: the chosen source label and the destination label, reason, and where it was registered e_old, e_new,
    distance: of the new displacement from the predicted one in xy, accepted, pair: its row of the gap's new tables), `counts`
    one word per FILL_REASONS (reasons 0 to 5 by the device's select, 6 to 8 by the host from the candidates' table)."""

    def __init__(self, before, plan_counts, retried, counts, ms=0.0):
        self.before, self.retried, self.ms = before, list(retried), float(ms)     # ms: the fill's wall time behind the tracks' read-back
        self.plan_counts = np.asarray(plan_counts, np.int64).reshape(4)
        self.counts = np.asarray(counts, np.int64).reshape(len(FILL_REASONS))

    def summary(self, after):
        return dict(missing=int(self.plan_counts[3]), retried=int(self.counts[:6].sum()), accepted=int(self.counts[0]),
                    reasons={name: int(v) for name, v in zip(FILL_REASONS, self.counts)},
                    observed_before=int(self.before.fit_counts[1]), observed_after=int(after.fit_counts[1]),
                    judged_before=int(self.before.fit_counts[2]), judged_after=int(after.fit_counts[2]))


class Tracks:
    """The tracks of one sample on the host (icpflow_object_tracks_fit's table, read back once)."""

    def __init__(self, rows, fit_counts, next_id, gaps, observation_ids, extend_counts, params):
        self.rows = np.asarray(rows, np.float64).reshape(-1, 16)
        self.fit_counts = np.asarray(fit_counts, np.int64).reshape(5)
        self.next_id, self.gaps, self.params = int(next_id), list(gaps), dict(params)
        self.observation_ids = [np.asarray(i, np.int64) for i in observation_ids]      # per gap, one per object row (-1: none)
        self.extend_counts = [np.asarray(c, np.int64).reshape(6) for c in extend_counts]
        self.repair = None                    # a Repair: set by pair_judges.frame_tracks(repair=True)
        self.fill = None                      # a Fill: set by pair_judges.frame_tracks(fill=True)

    def summary(self):
        _, observed, judged, consistent, moving = (int(v) for v in self.fit_counts)
        return dict(tracks=self.next_id, observed=observed, judged=judged, consistent=consistent, inconsistent=judged - consistent, moving=moving,
                    gaps=len(self.gaps), overflow=int(sum(int(c[5]) for c in self.extend_counts)))

    def as_list(self):
        """one dict per track with an observation, in the order of the ids"""
        out = []
        for r in self.rows:
            if r[1] <= 0:
                continue
            mask = int(r[2])
            out.append(dict(track=int(r[0]), observations=int(r[1]), gaps=[g for g in range(64) if mask >> g & 1], velocity=[float(v) for v in r[3:6]],
                            speed=float(r[6]), residual_max=float(r[7]), residual_rms=float(r[8]), moving=bool(r[9]), judged=bool(r[10]),
                            consistent=bool(r[11]), size=[float(v) for v in r[12:15]], points=int(r[15])))
        return out


def format_tracks(tracks):
    """`Tracks.as_list()` as lines of text"""
    lines = ["  track  views       vx       vy       vz    speed  residual  moving  judged  consistent   length    width   height  points"]
    yes = lambda b: "yes" if b else "no"    # noqa: E731
    for e in tracks:
        lines.append(f"{e['track']:7d}{e['observations']:7d}{e['velocity'][0]:9.2f}{e['velocity'][1]:9.2f}{e['velocity'][2]:9.2f}{e['speed']:9.2f}"
                     f"{e['residual_max']:10.3f}{yes(e['moving']):>8}{yes(e['judged']):>8}{yes(e['consistent']):>12}"
                     f"{e['size'][0]:9.2f}{e['size'][1]:9.2f}{e['size'][2]:9.2f}{e['points']:8d}")
    return lines


class LogTracks:
    """The tracks of one log on the host (icpflow_object_tracks_path's table, read back once): rows [tracks, 24], the table's
    five counts, and per file its observations ([P, 13], column 0 the track of every object row), its six carry counts and its
    six extend counts; frames [F, 12]: every file's destination frame in the log's frame; names: the files."""

    def __init__(self, rows, path_counts, next_id, observations, carry_counts, extend_counts, frames, names, source_rows, params):
        self.rows = np.asarray(rows, np.float64).reshape(-1, 24)
        self.path_counts = np.asarray(path_counts, np.int64).reshape(5)
        self.next_id, self.params, self.names = int(next_id), dict(params), list(names)
        self.observations = [np.asarray(o, np.float64).reshape(-1, 13) for o in observations]
        self.observation_ids = [np.rint(o[:, 0]).astype(np.int64) for o in self.observations]
        self.carry_counts = [np.asarray(c, np.int64).reshape(6) for c in carry_counts]
        self.extend_counts = [np.asarray(c, np.int64).reshape(6) for c in extend_counts]
        self.frames = np.asarray(frames, np.float64).reshape(-1, 12)
        self.source_rows = [int(n) for n in source_rows]

    def breaks(self):
        """the files at which the chain of ids started afresh (the carry found too few rows of the shared sweep)"""
        return [k for k, c in enumerate(self.carry_counts) if c[5]]

    def summary(self):
        observed, judged, smooth, moving = (int(v) for v in self.path_counts[1:])
        carried = sum(int(c[1]) for c in self.carry_counts if not c[5])
        return dict(files=len(self.observations), tracks=self.next_id, observed=observed, judged=judged, smooth=smooth, rough=judged - smooth,
                    moving=moving, breaks=len(self.breaks()), carried_rows=carried, rows=sum(self.source_rows[1:]),
                    overflow=int(sum(int(c[5]) for c in self.extend_counts)))

    def as_list(self):
        """one dict per track with a counted observation, in the order of the ids; `observations`: every object row of the
        track, file by file -- step, file, pair (its row in the file's tables), velocity in the log's frame (R d / seconds,
        float64 on the host)"""
        seen = {}
        for step, obs in enumerate(self.observations):
            R = self.frames[step, :9].reshape(3, 3)
            for pair, o in enumerate(obs):
                if o[0] >= 0:
                    seen.setdefault(int(o[0]), []).append(dict(step=step, file=self.names[step], pair=pair, velocity=[float(v) for v in (R @ o[3:6]) / o[2]]))
        out = []
        for r in self.rows:
            if r[1] <= 0:
                continue
            out.append(dict(track=int(r[0]), observations=seen.get(int(r[0]), []), counted=int(r[1]), first_step=int(r[2]), last_step=int(r[3]),
                            missing=int(r[4]), seconds=float(r[5]), path_length=float(r[6]), velocity=[float(v) for v in r[7:10]], speed=float(r[10]),
                            dv_max=float(r[11]), adjacent=int(r[12]), jump=float(r[13]), moving=bool(r[14]), judged=bool(r[15]), smooth=bool(r[16]),
                            size=[float(v) for v in r[17:20]], points=int(r[20]), start=[float(v) for v in r[21:24]]))
        return out


def format_log_tracks(tracks):
    """`LogTracks.as_list()` as lines of text"""
    lines = ["  track  steps  first   last  missing       vx       vy    speed   dv_max     jump  moving  judged  smooth   length    width   height  points"]
    yes = lambda b: "yes" if b else "no"    # noqa: E731
    for e in tracks:
        lines.append(f"{e['track']:7d}{e['counted']:7d}{e['first_step']:7d}{e['last_step']:7d}{e['missing']:9d}{e['velocity'][0]:9.2f}{e['velocity'][1]:9.2f}"
                     f"{e['speed']:9.2f}{e['dv_max']:9.3f}{e['jump']:9.3f}{yes(e['moving']):>8}{yes(e['judged']):>8}{yes(e['smooth']):>8}"
                     f"{e['size'][0]:9.2f}{e['size'][1]:9.2f}{e['size'][2]:9.2f}{e['points']:8d}")
    return lines

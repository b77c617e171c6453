"""Ego motion of a LiDAR sequence without poses -- drop-in for the reference's `egomotion` (utils_ego_motion.py:21-111),
which hands every frame to the kiss_icp package; here the method itself runs on the GPU behind the C ABI
(include/icpflow_hip.h "8(f) ego motion", csrc/ego.hip): scan-to-map odometry with a device-resident voxel map, every
iteration of a frame's registration in one launch, one read-back per frame.

    ego = egomotion(args)                        # constants: args.ego_config (a mapping) over the reference's defaults
    pose = ego.register_frame(frame, timestamps) # frame [n,>=3] (numpy or a device tensor) -> float64 [4,4], frame -> frame 0
    ego.poses                                    # the poses so far

The estimator's second configuration (config_kiss_icp.yaml's "advanced" block) is a mapping of its own, MOTION_DEFAULTS,
read from args.ego_motion and the `motion=` keyword: `deskew` (off, as in the reference's configuration), `mid_stamp`,
`fixed_threshold` (0 = adaptive).  With `deskew` on, `timestamps` -- one stamp per point, NORMALISED BY THE CALLER to
[0, 1] over the sweep, used as given -- moves every point by exp((stamp - mid_stamp) * log(inv(poses[-2]) poses[-1])) on
the GPU before the frame is registered.  None or a scalar (the reference's own call passes one constant per frame, for
which deskewing is a no-op by design) takes the plain path; so does an array with `deskew` off.
"""
import ctypes

import numpy as np
import torch

from . import _lib

# config_kiss_icp.yaml as the reference's scripts set it (data.max_range, data.min_range, mapping.voxel_size = max_range / 100,
# mapping.max_points_per_voxel, adaptive_threshold.*, registration.*)
DEFAULTS = dict(max_range=100.0, min_range=1.0, voxel_size=0.0, min_motion_th=0.1, initial_threshold=10.0,
                convergence=1e-4, max_points_per_voxel=20, max_iterations=500,
                # capacities of the device state (not the reference's): points of one frame, slots of a map table
                max_points=1 << 18, map_capacity=1 << 19)


# the "advanced" block of config_kiss_icp.yaml: data.deskew, adaptive_threshold.fixed_threshold; mid_stamp is the
# compensator's own constant (the frame's pose holds at the middle of the sweep)
MOTION_DEFAULTS = dict(deskew=False, mid_stamp=0.5, fixed_threshold=0.0)


def read_motion(args=None, motion=None):
    """MOTION_DEFAULTS <- args.ego_motion (a mapping) <- `motion` (a mapping)"""
    c = dict(MOTION_DEFAULTS)
    cfg = getattr(args, "ego_motion", None) if args is not None else None
    for src in (cfg or {}, motion or {}):
        for k, v in src.items():
            if k not in MOTION_DEFAULTS:
                raise TypeError(f"ego motion: unknown motion setting {k!r} (known: {sorted(MOTION_DEFAULTS)})")
            c[k] = v
    return c


def read_constants(args=None, **over):
    """DEFAULTS <- args.ego_config (a mapping, the counterpart of the reference's args.config file) <- keywords"""
    c = dict(DEFAULTS)
    cfg = getattr(args, "ego_config", None) if args is not None else None
    for src in (cfg or {}, over):
        for k, v in src.items():
            if k not in DEFAULTS:
                raise TypeError(f"ego motion: unknown constant {k!r} (known: {sorted(DEFAULTS)})")
            c[k] = v
    return c


class egomotion:
    def __init__(self, args=None, device=None, motion=None, **over):
        if not torch.cuda.is_available():
            raise RuntimeError("icp_flow_amd: ego motion needs a GPU (HIP) device -- there is no CPU path")
        self.args = args
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.constants = read_constants(args, **over)
        self.motion = read_motion(args, motion)
        self.corrected = None
        c = self.constants
        self._par = _lib.EgoParams.defaults(**{k: (int(v) if isinstance(DEFAULTS[k], int) else float(v)) for k, v in c.items()})
        need = int(_lib._L.icpflow_ego_state_bytes(ctypes.byref(self._par)))
        if need == 0:
            _lib.call("icpflow_ego_create", ctypes.byref(self._par), None, 0, None, ctypes.byref(_lib._p()))   # raises with the reason
        with torch.cuda.device(self.device):
            self._mem = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._h = _lib._p()
            _lib.call("icpflow_ego_create", ctypes.byref(self._par), _lib.ptr(self._mem), need, _lib.stream(self.device), ctypes.byref(self._h))
        self.voxel_size = c["voxel_size"] if c["voxel_size"] > 0 else c["max_range"] / 100.0
        if self.motion != MOTION_DEFAULTS:
            m = _lib.EgoMotionParams.defaults(deskew=int(bool(self.motion["deskew"])), mid_stamp=float(self.motion["mid_stamp"]),
                                              fixed_threshold=float(self.motion["fixed_threshold"]))
            try:
                _lib.call("icpflow_egomotion_set_params", self._h, ctypes.byref(m))
            except Exception:
                self.close()
                raise

    # ---- the reference's interface -------------------------------------------------------------------------------------------
    def register_frame(self, frame, timestamps=None):
        """-> the frame's pose.  `timestamps`: None, a scalar, or one stamp per point in [0, 1] (see the module's docstring);
        after a deskewed frame `self.corrected` is the frame as it was registered (float32 device tensor [n,3])."""
        pts = self._points(frame)
        n = int(pts.shape[0])
        out = (ctypes.c_double * 16)()
        stamps = self._stamps(timestamps, n) if self.motion["deskew"] else None
        with torch.cuda.device(self.device):
            if stamps is None:
                self.corrected = None
                _lib.call("icpflow_ego_register_frame", self._h, _lib.ptr(pts), n, out, _lib.stream(self.device))
            else:
                self.corrected = torch.empty((n, 3), dtype=torch.float32, device=self.device)
                _lib.call("icpflow_egomotion_register_frame_stamped", self._h, _lib.ptr(pts), _lib.ptr(stamps), n,
                          _lib.ptr(self.corrected), out, _lib.stream(self.device))
        return np.array(out, dtype=np.float64).reshape(4, 4)

    @property
    def poses(self):
        n = ctypes.c_int(0)
        _lib.call("icpflow_ego_poses", self._h, None, 0, ctypes.byref(n))
        buf = (ctypes.c_double * (16 * max(n.value, 1)))()
        _lib.call("icpflow_ego_poses", self._h, buf, n.value, ctypes.byref(n))
        return [np.array(buf[16 * j: 16 * j + 16], dtype=np.float64).reshape(4, 4) for j in range(n.value)]

    def reset(self):
        with torch.cuda.device(self.device):
            _lib.call("icpflow_ego_reset", self._h, _lib.stream(self.device))

    def frame_info(self):
        """what the last frame did: dict(frame_ds, source, iterations, final_dx, correspondences, sigma, map_voxels)"""
        buf = (ctypes.c_double * 8)()
        _lib.call("icpflow_ego_frame_info", self._h, buf)
        return dict(frame_ds=int(buf[0]), source=int(buf[1]), iterations=int(buf[2]), final_dx=float(buf[3]),
                    correspondences=int(buf[4]), sigma=float(buf[5]), map_voxels=int(buf[6]))

    # ---- the pieces (asynchronous on the current stream; they leave poses and threshold alone) -----------------------
    def deskew(self, frame, timestamps, poses=None):
        """step 0 alone -> float32 device tensor [n,3]: every point moved by exp((stamp - mid_stamp) xi), xi the twist
        between `poses` = (pose[-2], pose[-1]) or, without them, the state's last two poses (fewer than two: a copy).
        Whether `deskew` is on does not matter here."""
        pts = self._points(frame)
        n = int(pts.shape[0])
        stamps = self._stamps(timestamps, n)
        if stamps is None:
            raise RuntimeError("ego motion: deskew needs one stamp per point")
        g = None if poses is None else (ctypes.c_double * 32)(*np.asarray(poses, dtype=np.float64).reshape(32))
        res = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("icpflow_egomotion_deskew", self._h, _lib.ptr(pts), _lib.ptr(stamps), n, g, _lib.ptr(res), _lib.stream(self.device))
        return res

    def downsample(self, frame):
        """steps 1-2 -> (idx_ds, idx_source): int64 device tensors, rows of `frame` in ascending order"""
        pts = self._points(frame)
        n = int(pts.shape[0])
        idx = torch.empty((2, max(n, 1)), dtype=torch.int32, device=self.device)
        counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("icpflow_ego_downsample", self._h, _lib.ptr(pts), n, _lib.ptr(idx[0]), _lib.ptr(idx[1]), _lib.ptr(counts),
                      _lib.stream(self.device))
        k = counts.tolist()
        return idx[0, : k[0]].long(), idx[1, : k[1]].long()

    def register_step(self, source, guess, sigma):
        """step 5 alone against the map as it is -> float64 device tensor [20]: pose [16], iterations, final |dx|,
        correspondences of the last iteration, 0"""
        pts = self._points(source)
        g = (ctypes.c_double * 16)(*np.asarray(guess, dtype=np.float64).reshape(16))
        res = torch.empty(20, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("icpflow_ego_register_step", self._h, _lib.ptr(pts), int(pts.shape[0]), g, float(sigma), _lib.ptr(res),
                      _lib.stream(self.device))
        return res

    def map_add(self, frame_ds, pose):
        """the map half of step 6: `frame_ds` moved by `pose` enters the map, voxels out of range of the pose leave"""
        pts = self._points(frame_ds)
        g = (ctypes.c_double * 16)(*np.asarray(pose, dtype=np.float64).reshape(16))
        with torch.cuda.device(self.device):
            _lib.call("icpflow_ego_map_add", self._h, _lib.ptr(pts), int(pts.shape[0]), g, _lib.stream(self.device))

    def map_export(self):
        """-> (keys int64 [V], counts int32 [V], points float32 [V, max_points_per_voxel, 3]) of the live voxels, sorted by key"""
        per = int(self._par.max_points_per_voxel)
        num = torch.zeros(1, dtype=torch.int32, device=self.device)
        cap = 0
        while True:
            keys = torch.empty(max(cap, 1), dtype=torch.int64, device=self.device)
            counts = torch.empty(max(cap, 1), dtype=torch.int32, device=self.device)
            pts = torch.empty((max(cap, 1), per, 3), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.call("icpflow_ego_map_export", self._h, _lib.ptr(keys), _lib.ptr(counts), _lib.ptr(pts), cap, _lib.ptr(num),
                          _lib.stream(self.device))
            v = int(num.item())
            if v <= cap:
                break
            cap = v
        order = torch.argsort(keys[:v])
        return keys[:v][order], counts[:v][order], pts[:v][order]

    def _points(self, frame):
        if isinstance(frame, torch.Tensor):
            t = frame.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(frame)[:, 0:3], dtype=np.float32)).to(self.device)
        if t.dim() != 2 or t.shape[1] < 3:
            raise RuntimeError(f"ego motion: expected points [n,>=3], got {tuple(t.shape)}")
        return t[:, 0:3].to(torch.float32).contiguous()

    def _stamps(self, timestamps, n):
        """None for None or a scalar; else a float32 device tensor [n]"""
        if timestamps is None or (timestamps.dim() if isinstance(timestamps, torch.Tensor) else np.ndim(timestamps)) == 0:
            return None
        if isinstance(timestamps, torch.Tensor):
            t = timestamps.to(self.device)
        else:
            t = torch.from_numpy(np.ascontiguousarray(timestamps, dtype=np.float32)).to(self.device)
        if t.dim() != 1 or int(t.shape[0]) != n:
            raise RuntimeError(f"ego motion: expected {n} stamps, one per point, got {tuple(t.shape)}")
        return t.to(torch.float32).contiguous()

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            _lib._L.icpflow_ego_destroy(h)
            self._h = _lib._p()

    __del__ = close


def estimate_poses(frames, args=None, device=None, timestamps=None, motion=None, **over):
    """Poses of a sequence of frames (each [n,>=3], sensor coordinates) -> float64 [F,4,4], frame j -> frame 0.
    `timestamps`: one array of per-point stamps per frame, used when `deskew` is on (args.ego_motion / `motion`)."""
    if timestamps is not None and len(timestamps) != len(frames):
        raise ValueError(f"ego motion: {len(timestamps)} arrays of stamps for {len(frames)} frames")
    c = read_constants(args, **over)
    if "max_points" not in over and "max_points" not in (getattr(args, "ego_config", None) or {}):
        c["max_points"] = max(1024, max((len(f) for f in frames), default=1))      # the state as small as the sequence allows
    ego = egomotion(None, device, read_motion(args, motion), **c)
    try:
        stamps = timestamps if timestamps is not None else [None] * len(frames)
        return np.stack([ego.register_frame(f, s) for f, s in zip(frames, stamps)]) if len(frames) else np.zeros((0, 4, 4))
    finally:
        ego.close()

"""Host-side mirror of the odometry-fused local obstacle map (include/jn_localmap.h) over libjn_stereo.so.

Everything else this package produces is a function of one disparity map in the robot frame of that instant.  This mode, defined in
include/jn_localmap.h, accumulates frames over time in a FIXED frame using the robot's pose: an int16 log-odds grid that is raised where
obstacle pixels fell, lowered where floor pixels fell, and kept for what has left the field of view; `grid` is its reading in the
nav_msgs/OccupancyGrid convention (100 / 0 / -1).  The thresholds' defaults are untuned guesses."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ScanParams
from .costmap import OCCUPIED, FREE, UNKNOWN, MAX_CELLS  # noqa: F401
from .device import DeviceArray
from .subpix import F32, I16, I16_SUB, FORMAT_DTYPES  # noqa: F401

MAX_BATCH = 256


class Pose2D(C.Structure):
    """jn_pose2d: the robot in the fixed frame (metres, radians)."""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("theta", C.c_double)]


class LocalMapParams(C.Structure):
    """jn_localmap_params."""
    _fields_ = [("resolution", C.c_double), ("cells_x", C.c_int32), ("cells_y", C.c_int32), ("min_hits", C.c_int32), ("min_floor", C.c_int32),
                ("l_hit", C.c_int32), ("l_miss", C.c_int32), ("l_min", C.c_int32), ("l_max", C.c_int32), ("occ_thresh", C.c_int32),
                ("free_thresh", C.c_int32), ("format", C.c_int32), ("min_q", C.c_int32)]


LOCALMAP_EXPORTS = ["jn_localmap_params_default", "jn_localmap_create", "jn_localmap_destroy", "jn_localmap_reset", "jn_localmap_recenter",
                    "jn_localmap_window", "jn_localmap_update", "jn_localmap_read"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_localmap_bound", False):
        vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
        LP = C.POINTER(LocalMapParams)
        L.jn_localmap_params_default.argtypes = [LP, i32]
        L.jn_localmap_params_default.restype = None
        L.jn_localmap_create.argtypes = [LP, i32, i32, C.POINTER(vp)]
        L.jn_localmap_destroy.argtypes = [vp]
        L.jn_localmap_destroy.restype = None
        L.jn_localmap_reset.argtypes = [vp]
        L.jn_localmap_recenter.argtypes = [vp, f64, f64]
        L.jn_localmap_window.argtypes = [vp, C.POINTER(C.c_int64 * 2), C.POINTER(f64 * 2)]
        L.jn_localmap_update.argtypes = [vp, C.POINTER(ScanParams), i32, C.POINTER(Pose2D), vp, i32, i32, vp, vp]
        L.jn_localmap_read.argtypes = [vp, vp, vp]
        L._localmap_bound = True
    return L


def localmap_params(fmt, **overrides):
    """The defaults (0.05 m cells, 256 x 256, min_hits 3, min_floor 3, l_hit 4, l_miss 1, l_min -8, l_max 16, occ_thresh 4, free_thresh -2,
    min_q 32 — untuned guesses) for a format, with fields overridden by keyword."""
    p = LocalMapParams()
    _bind().jn_localmap_params_default(C.byref(p), fmt)
    for k, v in overrides.items():
        if k not in dict(p._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class Window:
    """Where the map's cells are in the fixed frame: cell (0, 0) has the global index g0 and the corner `origin` (metres)."""

    def __init__(self, g0, origin, resolution, cells_x, cells_y):
        self.g0, self.origin, self.resolution, self.cells_x, self.cells_y = tuple(g0), tuple(origin), resolution, cells_x, cells_y

    def __repr__(self):
        return "Window(g0=%s, origin=%s, %dx%d @ %g)" % (self.g0, self.origin, self.cells_x, self.cells_y, self.resolution)


def _as_poses(poses):
    if isinstance(poses, Pose2D):
        poses = [poses]
    arr = (Pose2D * len(poses))()
    for k, p in enumerate(poses):
        arr[k] = p if isinstance(p, Pose2D) else Pose2D(*[float(v) for v in p])
    return arr


class LocalMap:
    """A jn_localmap handle: the rolling log-odds grid on one device.  A context manager; one thread at a time.

        with LocalMap(localmap_params(F32), max_batch=4) as m:
            m.follow(pose, margin_cells=64)            # host policy: recentre when the robot nears the window's edge
            m.update(sp, [pose], dD1, W, H)            # after the matcher slot's wait
            log_odds, grid = m.read()
    """

    def __init__(self, params, max_batch=1, device=0):
        self._h = None
        self.params, self.max_batch, self.device = params, max_batch, device
        h = C.c_void_p()
        _lib.check(_bind().jn_localmap_create(C.byref(params), max_batch, device, C.byref(h)), "jn_localmap_create")
        self._h = h

    def close(self):
        if self._h:
            _bind().jn_localmap_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Every cell unknown (L = 0), the window recentred on (0, 0)."""
        _lib.check(_bind().jn_localmap_reset(self._h), "jn_localmap_reset")

    def recenter(self, x, y):
        """The window's centre cell becomes the cell of (x, y); cells in both windows keep their log-odds, entering cells are 0."""
        _lib.check(_bind().jn_localmap_recenter(self._h, x, y), "jn_localmap_recenter")

    def window(self):
        g0, org = (C.c_int64 * 2)(), (C.c_double * 2)()
        _lib.check(_bind().jn_localmap_window(self._h, C.byref(g0), C.byref(org)), "jn_localmap_window")
        p = self.params
        return Window((int(g0[0]), int(g0[1])), (float(org[0]), float(org[1])), p.resolution, p.cells_x, p.cells_y)

    def follow(self, pose, margin_cells):
        """Host policy, not part of the definition: recentre on the robot when its cell is more than `margin_cells` from the window's
        centre cell along x or y.  Returns whether the window moved."""
        x, y = (pose.x, pose.y) if isinstance(pose, Pose2D) else (pose[0], pose[1])
        p, g0 = self.params, self.window().g0
        off_x = math.floor(x / p.resolution) - (g0[0] + p.cells_x // 2)
        off_y = math.floor(y / p.resolution) - (g0[1] + p.cells_y // 2)
        if max(abs(off_x), abs(off_y)) <= margin_cells:
            return False
        self.recenter(x, y)
        return True

    def update(self, sp, poses, dDisp, width, height, dObst=None, dFloor=None):
        """len(poses) maps [n][height][width] (device pointer, the handle's format), one pose (Pose2D or (x, y, theta)) per map, applied in
        index order.  dObst / dFloor: optional device pointers for the frames' saturated counts [n][cells_y][cells_x] u16.  Synchronous
        (jn_localmap_update)."""
        arr = _as_poses(poses)
        _lib.check(_bind().jn_localmap_update(self._h, C.byref(sp), len(arr), arr, dDisp, width, height, dObst, dFloor), "jn_localmap_update")

    def read_device(self, dLogOdds=None, dGrid=None):
        """The state into device memory: dLogOdds [cells_y][cells_x] int16, dGrid int8 (either may be None)."""
        _lib.check(_bind().jn_localmap_read(self._h, dLogOdds, dGrid), "jn_localmap_read")

    def read(self):
        """-> (log_odds [cells_y][cells_x] int16, grid [cells_y][cells_x] int8) as numpy arrays, window order."""
        p = self.params
        dL = DeviceArray((p.cells_y, p.cells_x), np.int16, self.device); dG = DeviceArray((p.cells_y, p.cells_x), np.int8, self.device)
        try:
            self.read_device(dL.ptr, dG.ptr)
            return dL.numpy(), dG.numpy()
        finally:
            dL.free(); dG.free()


def occupancy_grid_message(grid, window, seq=0, frame_id="odom"):
    """The nav_msgs/OccupancyGrid fields of the map's grid [cells_y][cells_x] int8 in the fixed frame — the counterpart of
    costmap.occupancy_grid_message, whose grid is in the robot frame."""
    grid = np.ascontiguousarray(grid, np.int8)
    if grid.shape != (window.cells_y, window.cells_x):
        raise ValueError("grid is %s, the window says (%d, %d)" % (grid.shape, window.cells_y, window.cells_x))
    return {
        "header": {"seq": int(seq), "frame_id": frame_id},
        "info": {"resolution": np.float32(window.resolution), "width": int(window.cells_x), "height": int(window.cells_y),
                 "origin": {"position": {"x": float(window.origin[0]), "y": float(window.origin[1]), "z": 0.0},
                            "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
        "data": grid.reshape(-1).copy(),
    }

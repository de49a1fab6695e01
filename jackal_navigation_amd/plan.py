"""Host-side mirror of the local planner (include/jn_plan.h) over libjn_stereo.so.

Two pieces, both defined in include/jn_plan.h: the CLEARANCE FIELD of an occupancy grid (u16, the exact squared distance in cells to the
nearest obstacle cell within a radius, 65535 beyond it) and a ROLLOUT of candidate arcs (v, omega) through it from the robot's pose, with a
host-side choice among them toward a goal.  It reads every grid the package makes: the robot-frame grids of costmap / subpix (zero pose,
the costmap's origin) and LocalMap's grid in the fixed frame (the window's origin).  The velocity limits are the reference's
(navigate.cpp:33-34); every other default is an untuned guess."""
import ctypes as C

import numpy as np

from . import _lib
from .costmap import MAX_CELLS  # noqa: F401
from .device import DeviceArray
from .localmap import Pose2D, _as_poses

FAR = 65535
MAX_RADIUS = 255
MAX_BATCH = 256
OK, BLOCKED = 0, 1


class PlanParams(C.Structure):
    """jn_plan_params."""
    _fields_ = [("v_max", C.c_double), ("w_max", C.c_double), ("horizon", C.c_double), ("robot_radius", C.c_double), ("w_goal", C.c_double),
                ("w_clear", C.c_double), ("w_speed", C.c_double), ("clear_cap", C.c_double), ("n_v", C.c_int32), ("n_w", C.c_int32),
                ("steps", C.c_int32), ("reserved", C.c_int32)]


class PlanRecord(C.Structure):
    """jn_plan_record."""
    _fields_ = [("t_end", C.c_int32), ("t_hit", C.c_int32), ("min_d2", C.c_int32), ("last_cell", C.c_int32)]


class PlanCmd(C.Structure):
    """jn_plan_cmd."""
    _fields_ = [("v", C.c_double), ("w", C.c_double), ("candidate", C.c_int32), ("status", C.c_int32)]


RECORD_DTYPE = np.dtype([("t_end", np.int32), ("t_hit", np.int32), ("min_d2", np.int32), ("last_cell", np.int32)])

PLAN_EXPORTS = ["jn_clearance", "jn_plan_params_default", "jn_plan_templates", "jn_plan_create", "jn_plan_destroy", "jn_plan_evaluate",
                "jn_plan_choose", "jn_plan_command"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_plan_bound", False):
        vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
        PP = C.POINTER(PlanParams)
        L.jn_clearance.argtypes = [i32, i32, vp, i32, i32, i32, i32, vp]
        L.jn_plan_params_default.argtypes = [PP]
        L.jn_plan_params_default.restype = None
        L.jn_plan_templates.argtypes = [PP, vp, vp, vp]
        L.jn_plan_create.argtypes = [PP, f64, i32, i32, i32, i32, C.POINTER(vp)]
        L.jn_plan_destroy.argtypes = [vp]
        L.jn_plan_destroy.restype = None
        L.jn_plan_evaluate.argtypes = [vp, i32, vp, C.POINTER(f64 * 2), C.POINTER(Pose2D), vp]
        L.jn_plan_choose.argtypes = [PP, f64, vp, C.POINTER(Pose2D), C.POINTER(f64 * 2), C.POINTER(PlanCmd)]
        L.jn_plan_command.argtypes = [vp, i32, vp, C.POINTER(f64 * 2), C.POINTER(Pose2D), vp, vp, vp]
        L._plan_bound = True
    return L


def plan_params(**overrides):
    """The defaults (v_max 0.6, w_max 1.3, horizon 2.0, robot_radius 0.3, w_goal 1.0, w_clear 0.5, w_speed 0.1, clear_cap 1.0, n_v 3,
    n_w 11, steps 20 — untuned guesses apart from the two limits) with fields overridden by keyword."""
    p = PlanParams()
    _bind().jn_plan_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(p._fields_):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def clearance(grid, radius, unknown_is_obstacle=0, n=None, cells_x=None, cells_y=None, dD2=None, device=0):
    """The clearance field (jn_clearance; synchronous).  `grid` is either a numpy int8 array [cells_y][cells_x] or [n][cells_y][cells_x]
    — uploaded, and the field returned as a numpy u16 array of the same shape — or a device pointer to n grids, with n, cells_x, cells_y
    and the output pointer dD2 ([n][cells_y][cells_x] u16) given."""
    L = _bind()
    if isinstance(grid, np.ndarray):
        g = np.ascontiguousarray(grid, np.int8)
        if g.ndim not in (2, 3):
            raise ValueError("a grid is [cells_y][cells_x] or [n][cells_y][cells_x]")
        shape = g.shape if g.ndim == 3 else (1,) + g.shape
        dG = DeviceArray.from_numpy(g, device); dD = DeviceArray(g.shape, np.uint16, device)
        try:
            _lib.check(L.jn_clearance(device, shape[0], dG.ptr, shape[2], shape[1], unknown_is_obstacle, radius, dD.ptr), "jn_clearance")
            return dD.numpy()
        finally:
            dG.free(); dD.free()
    if n is None or cells_x is None or cells_y is None or dD2 is None:
        raise ValueError("a device grid needs n, cells_x, cells_y and dD2")
    _lib.check(L.jn_clearance(device, n, grid, cells_x, cells_y, unknown_is_obstacle, radius, dD2), "jn_clearance")
    return None


def localmap_clearance(m, radius, unknown_is_obstacle=0, dD2=None):
    """The clearance field of a LocalMap's current grid without a host round trip: the grid is read on the device (jn_localmap_read) and
    transformed there.  dD2: a device pointer [cells_y][cells_x] u16 to fill (None is returned), or None: a DeviceArray the caller frees."""
    p = m.params
    dG = DeviceArray((p.cells_y, p.cells_x), np.int8, m.device)
    out = None
    try:
        m.read_device(None, dG.ptr)
        if dD2 is None:
            out = DeviceArray((p.cells_y, p.cells_x), np.uint16, m.device)
        clearance(dG.ptr, radius, unknown_is_obstacle, 1, p.cells_x, p.cells_y, out.ptr if out is not None else dD2, m.device)
        return out
    finally:
        dG.free()


def templates(params):
    """-> (v [K], w [K], xy [K][steps][2]) float64 of the candidates (jn_plan_templates; host only, needs no device)."""
    K, T = params.n_v * params.n_w, params.steps
    if K < 1 or T < 1 or K > 16 * 65 or T > 128:
        raise _lib.JnError(_lib.JN_ERR_INVALID, "jn_plan_templates")
    v, w, xy = np.empty(K), np.empty(K), np.empty((K, T, 2))
    _lib.check(_bind().jn_plan_templates(C.byref(params), v.ctypes.data, w.ctypes.data, xy.ctypes.data), "jn_plan_templates")
    return v, w, xy


def _pose(pose):
    return pose if isinstance(pose, Pose2D) else Pose2D(*[float(x) for x in pose])


def choose(params, resolution, records, pose, goal):
    """The choice among one frame's records (a RECORD_DTYPE array [K]) toward goal (x, y) -> PlanCmd (jn_plan_choose; host only)."""
    rec = np.ascontiguousarray(records, RECORD_DTYPE)
    if rec.shape != (params.n_v * params.n_w,):
        raise ValueError("records must be [n_v * n_w]")
    cmd = PlanCmd()
    g = (C.c_double * 2)(float(goal[0]), float(goal[1]))
    q = _pose(pose)
    _lib.check(_bind().jn_plan_choose(C.byref(params), resolution, rec.ctypes.data, C.byref(q), C.byref(g), C.byref(cmd)), "jn_plan_choose")
    return cmd


class Plan:
    """A jn_plan handle: the candidates' templates and the per-call buffers on one device.  A context manager; one thread at a time.

        with Plan(plan_params(), resolution=0.05, cells_x=256, cells_y=256) as pl:
            field = plan.localmap_clearance(m, radius=20)                         # device, no host round trip
            cmd, = pl.command(field.ptr, m.window().origin, [pose], [goal])
            msg = plan.twist_message(cmd)
    """

    def __init__(self, params, resolution, cells_x, cells_y, max_batch=1, device=0):
        self._h = None
        self.params, self.resolution, self.cells_x, self.cells_y = params, resolution, cells_x, cells_y
        self.max_batch, self.device = max_batch, device
        self.K = params.n_v * params.n_w
        h = C.c_void_p()
        _lib.check(_bind().jn_plan_create(C.byref(params), resolution, cells_x, cells_y, max_batch, device, C.byref(h)), "jn_plan_create")
        self._h = h

    def close(self):
        if self._h:
            _bind().jn_plan_destroy(self._h)
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

    def evaluate(self, dD2, origin, poses):
        """len(poses) fields dD2 [n][cells_y][cells_x] u16 (device pointer) of grids with the corner `origin` (x, y), one pose per field
        -> the records, a RECORD_DTYPE array [n][K].  Synchronous (jn_plan_evaluate)."""
        arr = _as_poses(poses)
        rec = np.empty((len(arr), self.K), RECORD_DTYPE)
        org = (C.c_double * 2)(float(origin[0]), float(origin[1]))
        _lib.check(_bind().jn_plan_evaluate(self._h, len(arr), dD2, C.byref(org), arr, rec.ctypes.data), "jn_plan_evaluate")
        return rec

    def command(self, dD2, origin, poses, goals, with_records=False):
        """evaluate, then the choice per frame toward goals [(x, y)] in the poses' frame -> a list of PlanCmd (and the records with
        with_records).  Synchronous (jn_plan_command)."""
        arr = _as_poses(poses)
        n = len(arr)
        g = np.ascontiguousarray(goals, np.float64).reshape(n, 2)
        cmds = (PlanCmd * n)()
        rec = np.empty((n, self.K), RECORD_DTYPE) if with_records else None
        org = (C.c_double * 2)(float(origin[0]), float(origin[1]))
        _lib.check(_bind().jn_plan_command(self._h, n, dD2, C.byref(org), arr, g.ctypes.data, cmds, rec.ctypes.data if with_records else None),
                   "jn_plan_command")
        out = [PlanCmd(c.v, c.w, c.candidate, c.status) for c in cmds]
        return (out, rec) if with_records else out


def twist_message(cmd):
    """The geometry_msgs/Twist fields of a command (linear.x, angular.z: what the reference publishes at navigate.cpp:338-340) — the
    counterpart of occupancy_grid_message.  A blocked command is the zero twist."""
    return {"linear": {"x": float(cmd.v), "y": 0.0, "z": 0.0}, "angular": {"x": 0.0, "y": 0.0, "z": float(cmd.w)}}

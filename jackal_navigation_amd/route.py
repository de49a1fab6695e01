"""Host-side mirror of the cost-to-go field (include/jn_route.h) over libjn_stereo.so.

The FIELD: for every cell of a clearance field the least cost of a path through free space to a goal (u16; 5 per axis step, 7 per
diagonal step, a penalty per cell entered near an obstacle; 65535 where there is none), made on the device; and plan.Plan's arc ROLLOUT
scored by that field in place of the straight line to the goal, so that the planner drives out of a dead end the map remembers instead of
reporting BLOCKED from inside it.  Every default is an untuned guess."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .device import DeviceArray
from .localmap import Pose2D, _as_poses
from .plan import RECORD_DTYPE, PlanCmd, PlanParams, clearance
from .plan import _bind as _bind_plan

UNREACHED = 65535
MAX_R2 = 65025
MAX_NEAR_RADIUS = 255
MAX_NEAR_PENALTY = 64
MAX_GOAL_RADIUS = 16
OK, NO_ROUTE = 0, 1
FORM_WHOLE, FORM_TILED = 0, 1


class RouteParams(C.Structure):
    """jn_route_params."""
    _fields_ = [("near_radius", C.c_int32), ("near_penalty", C.c_int32), ("goal_radius", C.c_int32), ("reserved", C.c_int32)]


class RouteStats(C.Structure):
    """jn_route_stats."""
    _fields_ = [("form", C.c_int32), ("launches", C.c_int32), ("rounds", C.c_int32), ("reserved", C.c_int32)]


ROUTE_EXPORTS = ["jn_route_params_default", "jn_route_goal_cell", "jn_route_field", "jn_route_evaluate", "jn_route_choose", "jn_route_command",
                 "jn_route_trace"]


def _bind():
    L = _bind_plan()
    if not getattr(L, "_route_bound", False):
        vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
        RP, PP, D2 = C.POINTER(RouteParams), C.POINTER(PlanParams), C.POINTER(f64 * 2)
        L.jn_route_params_default.argtypes = [RP]
        L.jn_route_params_default.restype = None
        L.jn_route_goal_cell.argtypes = [f64, i32, i32, D2, D2, C.POINTER(i32 * 2)]
        L.jn_route_field.argtypes = [i32, i32, vp, i32, i32, i32, RP, vp, vp, vp, C.POINTER(RouteStats)]
        L.jn_route_evaluate.argtypes = [vp, i32, vp, vp, D2, C.POINTER(Pose2D), vp, vp]
        L.jn_route_choose.argtypes = [PP, f64, vp, vp, C.POINTER(PlanCmd)]
        L.jn_route_command.argtypes = [vp, i32, vp, vp, D2, C.POINTER(Pose2D), vp, vp, vp]
        L.jn_route_trace.argtypes = [vp, vp, i32, i32, i32, RP, i32, i32, vp, i32, C.POINTER(i32), C.POINTER(i32)]
        L._route_bound = True
    return L


def route_params(**overrides):
    """The defaults (near_radius 10, near_penalty 3, goal_radius 2 — untuned guesses) with fields overridden by keyword."""
    rp = RouteParams()
    _bind().jn_route_params_default(C.byref(rp))
    for k, v in overrides.items():
        if k not in dict(rp._fields_):
            raise AttributeError(k)
        setattr(rp, k, v)
    return rp


def r2_of(plan_params, resolution):
    """jn_plan.h's r2: floor((robot_radius / resolution)^2), the quotient and the product in double."""
    q = plan_params.robot_radius / resolution
    return int(math.floor(q * q))


def min_clearance_radius(r2, params):
    """The smallest radius a clearance field may be made with for this r2 and these parameters: beyond its radius the field says FAR,
    and a hit or a penalty further out would silently vanish (jn_route.h "radius")."""
    root = math.isqrt(r2)
    return max(root + (root * root < r2), params.near_radius, 1)


def goal_cell(resolution, cells_x, cells_y, origin, goal):
    """A goal (x, y) in the frame of the grid whose corner is `origin` -> its cell (ix, iy), clamped onto the grid (jn_route_goal_cell;
    host only)."""
    cell = (C.c_int32 * 2)()
    org = (C.c_double * 2)(float(origin[0]), float(origin[1]))
    g = (C.c_double * 2)(float(goal[0]), float(goal[1]))
    _lib.check(_bind().jn_route_goal_cell(resolution, cells_x, cells_y, C.byref(org), C.byref(g), C.byref(cell)), "jn_route_goal_cell")
    return int(cell[0]), int(cell[1])


def _goal_array(goal_cells, n):
    g = np.ascontiguousarray(goal_cells, np.int32)
    if g.size % 2 or g.ndim > 2:
        raise ValueError("goal_cells must be [n][2] (ix, iy)")
    g = g.reshape(-1, 2)
    if n >= 1 and len(g) != n:                                          # (an n out of range is the library's to refuse)
        raise ValueError("goal_cells must be [n][2] (ix, iy)")
    return g


def costtogo(d2, r2, params, goal_cells, n=None, cells_x=None, cells_y=None, dTogo=None, device=0, with_stats=False):
    """The cost-to-go field (jn_route_field; synchronous).  `d2` is either a numpy u16 clearance field [cells_y][cells_x] or
    [n][cells_y][cells_x] — uploaded, and (g, seeds) returned: g a numpy u16 array of the same shape, seeds an int32 array [n] — or a
    device pointer to n fields, with n, cells_x, cells_y and the output pointer dTogo given (seeds is returned).  goal_cells: [n][2]
    (ix, iy).  with_stats appends the RouteStats of the call."""
    L = _bind()
    st = RouteStats()
    if isinstance(d2, np.ndarray):
        f = np.ascontiguousarray(d2, np.uint16)
        if f.ndim not in (2, 3):
            raise ValueError("a field is [cells_y][cells_x] or [n][cells_y][cells_x]")
        shape = f.shape if f.ndim == 3 else (1,) + f.shape
        goals = _goal_array(goal_cells, shape[0])
        seeds = np.zeros(shape[0], np.int32)
        dD = DeviceArray.from_numpy(f, device); dG = DeviceArray(f.shape, np.uint16, device)
        try:
            _lib.check(L.jn_route_field(device, shape[0], dD.ptr, shape[2], shape[1], r2, C.byref(params), goals.ctypes.data, dG.ptr,
                                        seeds.ctypes.data, C.byref(st)), "jn_route_field")
            return (dG.numpy(), seeds, st) if with_stats else (dG.numpy(), seeds)
        finally:
            dD.free(); dG.free()
    if n is None or cells_x is None or cells_y is None or dTogo is None:
        raise ValueError("a device field needs n, cells_x, cells_y and dTogo")
    goals = _goal_array(goal_cells, n)
    seeds = np.zeros(n, np.int32)
    _lib.check(L.jn_route_field(device, n, d2, cells_x, cells_y, r2, C.byref(params), goals.ctypes.data, dTogo, seeds.ctypes.data, C.byref(st)),
               "jn_route_field")
    return (seeds, st) if with_stats else seeds


def localmap_costtogo(m, plan_params, goal, params=None, radius=None, unknown_is_obstacle=0):
    """Clearance field and cost-to-go field of a LocalMap's current grid toward `goal` (x, y) in the map's fixed frame, without a host round
    trip: the grid is read, transformed and relaxed on the device.  -> (dD2, dTogo, seeds, cell): two DeviceArrays
    [cells_y][cells_x] u16 the caller frees, the number of seed cells (0: the goal is blocked) and the goal's cell.  `radius`: the
    clearance radius, by default and at least min_clearance_radius(r2, params)."""
    from .plan import localmap_clearance
    params = params if params is not None else route_params()
    p = m.params
    r2 = r2_of(plan_params, p.resolution)
    need = min_clearance_radius(r2, params)
    radius = need if radius is None else radius
    if radius < need:
        raise ValueError("a clearance radius of %d cells is below the %d this r2 and near_radius need (jn_route.h)" % (radius, need))
    cell = goal_cell(p.resolution, p.cells_x, p.cells_y, m.window().origin, goal)
    dD2 = localmap_clearance(m, radius, unknown_is_obstacle)
    dTogo = DeviceArray((p.cells_y, p.cells_x), np.uint16, m.device)
    try:
        seeds = costtogo(dD2.ptr, r2, params, [cell], 1, p.cells_x, p.cells_y, dTogo.ptr, m.device)
    except Exception:
        dD2.free(); dTogo.free()
        raise
    return dD2, dTogo, int(seeds[0]), cell


def grid_costtogo(grid, plan_params, resolution, goal_cells, params=None, radius=None, unknown_is_obstacle=0, device=0):
    """numpy occupancy grids [cells_y][cells_x] or [n][...] int8 -> (d2, g, seeds) as numpy arrays: plan.clearance with a radius of at
    least min_clearance_radius, then costtogo."""
    params = params if params is not None else route_params()
    r2 = r2_of(plan_params, resolution)
    need = min_clearance_radius(r2, params)
    radius = need if radius is None else radius
    if radius < need:
        raise ValueError("a clearance radius of %d cells is below the %d this r2 and near_radius need (jn_route.h)" % (radius, need))
    d2 = clearance(np.asarray(grid, np.int8), radius, unknown_is_obstacle, device=device)
    g, seeds = costtogo(d2, r2, params, goal_cells, device=device)
    return d2, g, seeds


def choose(plan_params, resolution, records, togo):
    """The choice among one frame's records (RECORD_DTYPE [K]) and togo values (u16 [K]) -> PlanCmd (jn_route_choose; host only)."""
    rec = np.ascontiguousarray(records, RECORD_DTYPE)
    tg = np.ascontiguousarray(togo, np.uint16)
    K = plan_params.n_v * plan_params.n_w
    if rec.shape != (K,) or tg.shape != (K,):
        raise ValueError("records and togo must be [n_v * n_w]")
    cmd = PlanCmd()
    _lib.check(_bind().jn_route_choose(C.byref(plan_params), resolution, rec.ctypes.data, tg.ctypes.data, C.byref(cmd)), "jn_route_choose")
    return cmd


def trace(g, d2, r2, params, start, capacity=None):
    """The path from the cell start = (ix, iy) down one frame's field: host copies g and d2 [cells_y][cells_x] u16 -> (cells, status),
    cells an int32 array of indices iy * cells_x + ix (empty with status NO_ROUTE).  capacity: the most cells to accept, by default the
    whole grid; a longer path is an error, never a cut one (jn_route_trace; host only)."""
    gg, dd = np.ascontiguousarray(g, np.uint16), np.ascontiguousarray(d2, np.uint16)
    if gg.ndim != 2 or gg.shape != dd.shape:
        raise ValueError("g and d2 must be [cells_y][cells_x]")
    cap = gg.size if capacity is None else int(capacity)
    cells = np.zeros(max(cap, 1), np.int32)
    length, status = C.c_int32(0), C.c_int32(0)
    _lib.check(_bind().jn_route_trace(gg.ctypes.data, dd.ctypes.data, gg.shape[1], gg.shape[0], r2, C.byref(params), int(start[0]), int(start[1]),
                                      cells.ctypes.data, cap, C.byref(length), C.byref(status)), "jn_route_trace")
    return cells[:length.value].copy(), status.value


def path_message(cells, origin, resolution, cells_x, frame_id="odom"):
    """The nav_msgs/Path fields of a traced path: one pose per cell at the cell's centre, identity orientation — next to
    plan.twist_message and occupancy_grid_message."""
    poses = []
    for c in np.asarray(cells, np.int64).tolist():
        ix, iy = c % cells_x, c // cells_x
        poses.append({"header": {"frame_id": frame_id},
                      "pose": {"position": {"x": float(origin[0]) + (ix + 0.5) * resolution, "y": float(origin[1]) + (iy + 0.5) * resolution, "z": 0.0},
                               "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}})
    return {"header": {"frame_id": frame_id}, "poses": poses}


class Route:
    """A plan.Plan scored by a cost-to-go field: the same handle, the same records, the goal reached through dTogo instead of (x, y).

        with Plan(pp, resolution=0.05, cells_x=256, cells_y=256) as pl:
            rt = route.Route(pl)
            dD2, dTogo, seeds, cell = route.localmap_costtogo(m, pp, goal)           # device, no host round trip
            cmd, = rt.command(dD2.ptr, dTogo.ptr, m.window().origin, [pose])
    """

    def __init__(self, plan):
        self.plan = plan

    def evaluate(self, dD2, dTogo, origin, poses):
        """-> (records RECORD_DTYPE [n][K], togo u16 [n][K]).  Synchronous (jn_route_evaluate)."""
        pl = self.plan
        arr = _as_poses(poses)
        rec = np.empty((len(arr), pl.K), RECORD_DTYPE)
        togo = np.empty((len(arr), pl.K), np.uint16)
        org = (C.c_double * 2)(float(origin[0]), float(origin[1]))
        _lib.check(_bind().jn_route_evaluate(pl._h, len(arr), dD2, dTogo, C.byref(org), arr, rec.ctypes.data, togo.ctypes.data), "jn_route_evaluate")
        return rec, togo

    def command(self, dD2, dTogo, origin, poses, with_records=False):
        """evaluate, then the choice per frame -> a list of PlanCmd (and the records and togo with with_records).  Synchronous
        (jn_route_command)."""
        pl = self.plan
        arr = _as_poses(poses)
        n = len(arr)
        cmds = (PlanCmd * n)()
        rec = np.empty((n, pl.K), RECORD_DTYPE) if with_records else None
        togo = np.empty((n, pl.K), np.uint16) if with_records else None
        org = (C.c_double * 2)(float(origin[0]), float(origin[1]))
        _lib.check(_bind().jn_route_command(pl._h, n, dD2, dTogo, C.byref(org), arr, cmds, rec.ctypes.data if with_records else None,
                                            togo.ctypes.data if with_records else None), "jn_route_command")
        out = [PlanCmd(c.v, c.w, c.candidate, c.status) for c in cmds]
        return (out, rec, togo) if with_records else out

"""Host-side mirror of the robot-frame obstacle costmap (include/jn_costmap.h) over libjn_stereo.so.

The reference publishes a 90-bin LaserScan (point_cloud.cpp:213-296) and, with -g, a point cloud; it has no occupancy grid.  This mode
is defined in include/jn_costmap.h: the u8 disparity map the scan bins, reprojected the same way, counted into a Cartesian grid in the
robot frame (`hits`) and classified occupied / free / unknown (`grid`, the nav_msgs/OccupancyGrid convention: 100 / 0 / -1)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ScanParams

OCCUPIED, FREE, UNKNOWN = 100, 0, -1
MAX_CELLS = 512


class CostmapParams(C.Structure):
    """jn_costmap_params."""
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("resolution", C.c_double),
                ("cells_x", C.c_int32), ("cells_y", C.c_int32), ("min_hits", C.c_int32), ("from_cloud", C.c_int32)]


COSTMAP_EXPORTS = ["jn_costmap_params_default", "jn_obstacle_costmap", "jn_elas_attach_costmap", "jn_sgm_attach_costmap", "jn_costmap_allreduce"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_costmap_bound", False):
        vp, i32 = C.c_void_p, C.c_int32
        L.jn_costmap_params_default.argtypes = [C.POINTER(CostmapParams)]
        L.jn_costmap_params_default.restype = None
        L.jn_obstacle_costmap.argtypes = [i32, C.POINTER(ScanParams), C.POINTER(CostmapParams), i32, vp, vp, i32, i32, vp, vp, vp]
        L.jn_elas_attach_costmap.argtypes = [vp, i32, C.POINTER(CostmapParams), vp, vp]
        L.jn_sgm_attach_costmap.argtypes = [vp, i32, C.POINTER(CostmapParams), vp, vp]
        L.jn_costmap_allreduce.argtypes = [vp, C.POINTER(ScanParams), C.POINTER(CostmapParams), i32, vp, vp, vp]
        L._costmap_bound = True
    return L


def costmap_params(**overrides):
    """The defaults (origin (0, -3.2), 0.05 m cells, 128 x 128, min_hits 3, from_cloud 0) with fields overridden by keyword."""
    cp = CostmapParams()
    _bind().jn_costmap_params_default(C.byref(cp))
    for k, v in overrides.items():
        if k not in dict(cp._fields_):
            raise AttributeError(k)
        setattr(cp, k, v)
    return cp


def obstacle_costmap(sp, cp, n, dDisp, dLut, width, height, dBins, dHits, dGrid, device=0):
    """n u8 maps (device) -> hits [n][cells_y][cells_x] u16 and grid (int8) on the device.  dLut may be None with cp.from_cloud = 1,
    dBins None leaves no cell free.  Synchronous (jn_obstacle_costmap)."""
    _lib.check(_bind().jn_obstacle_costmap(device, C.byref(sp), C.byref(cp), n, dDisp, dLut, width, height, dBins, dHits, dGrid), "jn_obstacle_costmap")


def attach(handle, slot, cp, dHits=None, dGrid=None):
    """From now on every scan batch submitted on `slot` of an Elas or Sgm handle also writes its costmap into dHits / dGrid (valid after
    the slot's wait).  cp = None detaches.  No batch may be in flight on the slot."""
    _lib.attach_tail(_bind(), "costmap", handle, slot, cp, dHits, dGrid, alternative="obstacle_costmap()")


def allreduce(comm, sp, cp, n, dBins, dHits, dGrid):
    """Cross-rig merge on a parallel.ScanComm: hits = element-wise maximum over the ranks, grid recomputed from them and dBins
    (jn_costmap_allreduce).  Not concurrently with a handle that has the communicator attached."""
    _lib.check(_bind().jn_costmap_allreduce(comm._h, C.byref(sp), C.byref(cp), n, dBins, dHits, dGrid), "jn_costmap_allreduce")


def occupancy_grid_message(grid, cp, seq=0):
    """The nav_msgs/OccupancyGrid fields of one frame's grid [cells_y][cells_x] int8 — the counterpart of node.laser_scan_message."""
    grid = np.ascontiguousarray(grid, np.int8)
    if grid.shape != (cp.cells_y, cp.cells_x):
        raise ValueError("grid is %s, the parameters say (%d, %d)" % (grid.shape, cp.cells_y, cp.cells_x))
    return {
        "header": {"seq": int(seq), "frame_id": "jackal"},
        "info": {"resolution": np.float32(cp.resolution), "width": int(cp.cells_x), "height": int(cp.cells_y),
                 "origin": {"position": {"x": float(cp.origin_x), "y": float(cp.origin_y), "z": 0.0},
                            "orientation": {"x": 0.0, "y": 0.0, "z": 0.0, "w": 1.0}}},
        "data": grid.reshape(-1).copy(),
    }

"""Host-side mirror of the sub-pixel navigation tail (include/jn_subpix.h) over libjn_stereo.so.

The reference rounds its disparity map to mono8 before reprojecting (point_cloud.cpp:422); node.py and costmap.py reproduce that for the
reference's own topics.  This mode, defined in include/jn_subpix.h, reprojects the disparity the matcher computed — ELAS's float map, the
SGM and block-matching modes' int16 maps (integer or 1/16 pixel) — into the obstacle scan, the costmap and the point cloud."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ScanParams
from .costmap import CostmapParams
from .device import DeviceArray

F32, I16, I16_SUB = 0, 1, 2                       # == ground.F32 / I16 / I16_SUB
MAX_Q = 16 * 4096
FORMAT_DTYPES = {F32: np.float32, I16: np.int16, I16_SUB: np.int16}


class SubpixParams(C.Structure):
    """jn_subpix_params."""
    _fields_ = [("format", C.c_int32), ("min_q", C.c_int32)]


SUBPIX_EXPORTS = ["jn_subpix_params_default", "jn_subpix_scan", "jn_subpix_costmap", "jn_subpix_point_cloud", "jn_elas_attach_subpix",
                  "jn_sgm_attach_subpix"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_subpix_bound", False):
        vp, i32 = C.c_void_p, C.c_int32
        SP, CP, FP = C.POINTER(ScanParams), C.POINTER(CostmapParams), C.POINTER(SubpixParams)
        L.jn_subpix_params_default.argtypes = [FP, i32]
        L.jn_subpix_params_default.restype = None
        L.jn_subpix_scan.argtypes = [i32, SP, FP, i32, vp, i32, i32, vp, vp]
        L.jn_subpix_costmap.argtypes = [i32, SP, CP, FP, i32, vp, i32, i32, vp, vp, vp, vp]
        L.jn_subpix_point_cloud.argtypes = [i32, SP, FP, vp, i32, i32, vp, C.POINTER(C.c_int64)]
        L.jn_elas_attach_subpix.argtypes = [vp, i32, CP, vp, vp, vp, vp]
        L.jn_sgm_attach_subpix.argtypes = [vp, i32, CP, vp, vp, vp, vp]
        L._subpix_bound = True
    return L


def subpix_params(fmt, **overrides):
    """The defaults (min_q = 32: d >= 2) for a format, with fields overridden by keyword."""
    fp = SubpixParams()
    _bind().jn_subpix_params_default(C.byref(fp), fmt)
    for k, v in overrides.items():
        if k not in dict(fp._fields_):
            raise AttributeError(k)
        setattr(fp, k, v)
    return fp


def subpix_scan(sp, fp, n, dDisp, width, height, dBins, dMeta, device=0):
    """n maps in fp.format (device) -> bins [n][sp.bins], meta [n][4] doubles on the device.  Synchronous (jn_subpix_scan)."""
    _lib.check(_bind().jn_subpix_scan(device, C.byref(sp), C.byref(fp), n, dDisp, width, height, dBins, dMeta), "jn_subpix_scan")


def subpix_costmap(sp, cp, fp, n, dDisp, width, height, dBins, dMeta, dHits, dGrid, device=0):
    """The scan and the costmap (hits [n][cells_y][cells_x] u16, grid int8) of the same maps in one pass.  Synchronous (jn_subpix_costmap)."""
    _lib.check(_bind().jn_subpix_costmap(device, C.byref(sp), C.byref(cp), C.byref(fp), n, dDisp, width, height, dBins, dMeta, dHits, dGrid),
               "jn_subpix_costmap")


def subpix_point_cloud(sp, fp, dDisp, width, height, device=0):
    """One map -> the robot-frame float32 xyz triples of its valid pixels [count][3] (numpy), in jn_point_cloud's order."""
    xyz = DeviceArray((height * width, 3), np.float32, device)
    cnt = C.c_int64(0)
    _lib.check(_bind().jn_subpix_point_cloud(device, C.byref(sp), C.byref(fp), dDisp, width, height, xyz.ptr, C.byref(cnt)), "jn_subpix_point_cloud")
    out = xyz.numpy()[:cnt.value].copy()
    xyz.free()
    return out


def attach(handle, slot, cp=None, dBins=None, dMeta=None, dHits=None, dGrid=None):
    """From now on every scan batch submitted on `slot` of an Elas or Sgm handle also writes the sub-pixel scan into dBins / dMeta and,
    with cp, the costmap into dHits / dGrid (valid after the slot's wait).  Everything None detaches.  No batch may be in flight on the
    slot."""
    _lib.attach_tail(_bind(), "subpix", handle, slot, cp, dBins, dMeta, dHits, dGrid, alternative="subpix_costmap()")

"""Host-side mirror of the ground-plane estimator (include/jn_ground.h) over libjn_stereo.so.

The reference gets the camera-to-robot transform XR / XT by hand (README step 3: six rqt_reconfigure sliders turned until the cloud's
ground lines up in rviz).  This mode, defined in include/jn_ground.h, measures it: the floor is the dominant plane in the lower half of
a disparity map; `estimate` fits it on the GPU (integer arithmetic, in disparity space), `extrinsics` turns one or more fits into XR / XT
next to a prior.  A plane fixes roll, pitch and height; yaw and XT.x / XT.y stay the prior's."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ScanParams

F32, I16, I16_SUB = 0, 1, 2
MAX_SIDE = 4096
MAX_HYPOTHESES = 1024
FORMAT_DTYPES = {F32: np.float32, I16: np.int16, I16_SUB: np.int16}


class GroundParams(C.Structure):
    """jn_ground_params."""
    _fields_ = [("roi_x0", C.c_int32), ("roi_y0", C.c_int32), ("roi_x1", C.c_int32), ("roi_y1", C.c_int32),
                ("hypotheses", C.c_int32), ("tol_q", C.c_int32), ("min_disp", C.c_int32), ("min_inliers", C.c_int32),
                ("seed", C.c_uint32), ("reserved", C.c_int32),
                ("min_inlier_frac", C.c_double), ("beta_min", C.c_double), ("alpha_max", C.c_double)]


class GroundPlane(C.Structure):
    """jn_ground_plane."""
    _fields_ = [("status", C.c_int32), ("best", C.c_int32), ("inliers", C.c_int64), ("valid", C.c_int64), ("sums", C.c_int64 * 10),
                ("a", C.c_double), ("b", C.c_double), ("c", C.c_double), ("rms", C.c_double),
                ("n_cam", C.c_double * 3), ("height_m", C.c_double)]


GROUND_EXPORTS = ["jn_ground_params_default", "jn_ground_estimate", "jn_ground_solve", "jn_ground_nominal_prior", "jn_ground_align",
                  "jn_ground_extrinsics"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_ground_bound", False):
        vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
        L.jn_ground_params_default.argtypes = [C.POINTER(GroundParams), i32, i32]
        L.jn_ground_params_default.restype = None
        L.jn_ground_estimate.argtypes = [i32, C.POINTER(ScanParams), C.POINTER(GroundParams), i32, vp, i32, i32, i32, C.POINTER(GroundPlane), vp, vp]
        L.jn_ground_solve.argtypes = [C.POINTER(ScanParams), C.POINTER(GroundParams), vp, i64, C.POINTER(GroundPlane)]
        L.jn_ground_nominal_prior.argtypes = [vp, vp]
        L.jn_ground_nominal_prior.restype = None
        L.jn_ground_align.argtypes = [vp, dbl, vp, vp, dbl, vp, vp, C.POINTER(dbl)]
        L.jn_ground_extrinsics.argtypes = [C.POINTER(GroundPlane), i32, C.POINTER(ScanParams), dbl, vp, vp, C.POINTER(dbl)]
        L._ground_bound = True
    return L


def ground_params(width, height, **overrides):
    """The defaults (lower half of the frame, K = 256, tol_q = 8, ...) with fields overridden by keyword."""
    gp = GroundParams()
    _bind().jn_ground_params_default(C.byref(gp), width, height)
    for k, v in overrides.items():
        if k not in dict(gp._fields_):
            raise AttributeError(k)
        setattr(gp, k, v)
    return gp


def estimate(sp, gp, n, dDisp, fmt, width, height, want_scores=False, device=0):
    """n maps on the device (F32 / I16 / I16_SUB) -> a list of n GroundPlane.  With want_scores also (scores [n][K] int32,
    hyps [n][K][4] int64).  Synchronous (jn_ground_estimate)."""
    planes = (GroundPlane * n)()
    K = gp.hypotheses
    scores = np.zeros((n, K), np.int32) if want_scores else None
    hyps = np.zeros((n, K, 4), np.int64) if want_scores else None
    _lib.check(_bind().jn_ground_estimate(device, C.byref(sp), C.byref(gp), n, dDisp, fmt, width, height, planes,
                                          scores.ctypes.data if want_scores else None, hyps.ctypes.data if want_scores else None),
               "jn_ground_estimate")
    out = list(planes)
    return (out, scores, hyps) if want_scores else out


def solve(sp, gp, sums, valid):
    """The plane, status and geometry of ten refit sums (jn_ground_solve; host only)."""
    s = np.ascontiguousarray(sums, np.int64)
    if s.shape != (10,):
        raise ValueError("sums must hold ten integers")
    out = GroundPlane()
    _lib.check(_bind().jn_ground_solve(C.byref(sp), C.byref(gp), s.ctypes.data, int(valid), C.byref(out)), "jn_ground_solve")
    return out


def nominal_prior():
    """(XR, XT) of a forward-looking camera: robot x = camera z, y = -camera x, z = -camera y."""
    XR, XT = np.zeros(9), np.zeros(3)
    _bind().jn_ground_nominal_prior(XR.ctypes.data, XT.ctypes.data)
    return XR.reshape(3, 3), XT


def align(n_cam, height_m, XR0, XT0, max_tilt_deg=30.0):
    """A measured floor (unit normal towards the camera, camera height) next to the prior XR0 / XT0 -> (XR, XT, tilt_deg)."""
    nv, r0, t0 = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (n_cam, XR0, XT0))
    if nv.size != 3 or r0.size != 9 or t0.size != 3:
        raise ValueError("n_cam and XT0 hold three numbers, XR0 nine")
    XR, XT, tilt = np.zeros(9), np.zeros(3), C.c_double(0.0)
    _lib.check(_bind().jn_ground_align(nv.ctypes.data, float(height_m), r0.ctypes.data, t0.ctypes.data, float(max_tilt_deg), XR.ctypes.data,
                                       XT.ctypes.data, C.byref(tilt)), "jn_ground_align")
    return XR.reshape(3, 3), XT, tilt.value


def extrinsics(planes, sp_prior, max_tilt_deg=30.0):
    """The joint estimate of the planes with status OK next to sp_prior's XR / XT -> (XR, XT, tilt_deg) (jn_ground_extrinsics)."""
    arr = (GroundPlane * len(planes))(*planes)
    XR, XT, tilt = np.zeros(9), np.zeros(3), C.c_double(0.0)
    _lib.check(_bind().jn_ground_extrinsics(arr, len(planes), C.byref(sp_prior), float(max_tilt_deg), XR.ctypes.data, XT.ctypes.data,
                                            C.byref(tilt)), "jn_ground_extrinsics")
    return XR.reshape(3, 3), XT, tilt.value

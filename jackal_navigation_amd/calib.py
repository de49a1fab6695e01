"""Host-side mirror of the calibration-file reader / writer (include/jn_calib.h) over libjn_stereo.so: the OpenCV FileStorage YAML
subset the reference's main() reads (K1, K2, D1, D2, R, T, XR, XT), without OpenCV."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import StereoCalib

K1, K2, D1, D2, R, T, XR, XT = (1 << i for i in range(8))
STEREO = 63

CALIB_EXPORTS = ["jn_calib_load_yaml", "jn_calib_save_yaml"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_calib_bound", False):
        vp = C.c_void_p
        L.jn_calib_load_yaml.argtypes = [C.c_char_p, C.POINTER(StereoCalib), vp, vp, C.POINTER(C.c_int32)]
        L.jn_calib_save_yaml.argtypes = [C.c_char_p, C.POINTER(StereoCalib), vp, vp]
        L._calib_bound = True
    return L


def load_calibration(path, calib_width=640, calib_height=360):
    """-> (StereoCalib, XR [3][3], XT [3], present).  The file does not hold the size the rig was calibrated at: say it here.
    XR / XT absent from the file come back as identity / zero; `present` is the bit mask of the entries found."""
    c = StereoCalib()
    c.calib_width, c.calib_height = calib_width, calib_height
    xr, xt, present = np.zeros(9), np.zeros(3), C.c_int32(0)
    _lib.check(_bind().jn_calib_load_yaml(os.fsencode(path), C.byref(c), xr.ctypes.data, xt.ctypes.data, C.byref(present)), "jn_calib_load_yaml")
    return c, xr.reshape(3, 3), xt, present.value


def save_calibration(path, calib, XR, XT):
    """Writes all eight entries with 17 significant digits: load_calibration(save_calibration(x)) == x bit for bit."""
    xr, xt = np.ascontiguousarray(XR, np.float64).reshape(-1), np.ascontiguousarray(XT, np.float64).reshape(-1)
    if xr.size != 9 or xt.size != 3:
        raise ValueError("XR holds nine numbers, XT three")
    _lib.check(_bind().jn_calib_save_yaml(os.fsencode(path), C.byref(calib), xr.ctypes.data, xt.ctypes.data), "jn_calib_save_yaml")

"""Host-side mirror of the disparity post-filter (include/jn_postfilter.h) over libjn_stereo.so.

ELAS cleans its own map; the SGM and block-matching modes stop at the L/R check.  This filter, defined in include/jn_postfilter.h, removes
the speckles that survive it — connected segments of fewer than `speckle_size` pixels, neighbours within `speckle_range_q` 1/16 pixel —
and optionally runs a 3x3 median over the valid pixels, on the int16 maps of both modes (integer or 1/16 pixel)."""
import ctypes as C

import numpy as np

from . import _lib

I16, I16_SUB = 1, 2                                # == subpix.I16 / I16_SUB; subpix.F32 is refused
MAX_SIDE, MAX_SPECKLE_SIZE, MAX_RANGE_Q = 8192, 1 << 24, 4096
MARKERS = {I16: -1, I16_SUB: -16}                  # what a removed pixel becomes: the matchers' own invalid values
STATS = ("valid", "segments", "speckles", "removed")


class PostfilterParams(C.Structure):
    """jn_postfilter_params."""
    _fields_ = [("format", C.c_int32), ("speckle_size", C.c_int32), ("speckle_range_q", C.c_int32), ("median", C.c_int32)]


POSTFILTER_EXPORTS = ["jn_postfilter_params_default", "jn_disparity_postfilter", "jn_sgm_attach_postfilter"]


def _bind():
    L = _lib.load()
    if not getattr(L, "_postfilter_bound", False):
        vp, i32 = C.c_void_p, C.c_int32
        FP = C.POINTER(PostfilterParams)
        L.jn_postfilter_params_default.argtypes = [FP, i32]
        L.jn_postfilter_params_default.restype = None
        L.jn_disparity_postfilter.argtypes = [i32, FP, i32, vp, i32, i32, vp, vp]
        L.jn_sgm_attach_postfilter.argtypes = [vp, i32, FP, vp]
        L._postfilter_bound = True
    return L


def postfilter_params(fmt, **overrides):
    """The defaults (speckle_size 200, speckle_range_q 16 = one pixel, median 0) for a format, with fields overridden by keyword."""
    fp = PostfilterParams()
    _bind().jn_postfilter_params_default(C.byref(fp), fmt)
    for k, v in overrides.items():
        if k not in dict(fp._fields_):
            raise AttributeError(k)
        setattr(fp, k, v)
    return fp


def disparity_postfilter(fp, n, dIn, width, height, dOut=None, dStats=None, device=0):
    """n int16 maps in fp.format (device) -> the filtered maps in dOut (None: in place) and, with dStats [n][4] uint32, per map the valid
    pixels on input, the segments, the speckle segments and the pixels removed.  Synchronous (jn_disparity_postfilter)."""
    _lib.check(_bind().jn_disparity_postfilter(device, C.byref(fp), n, dIn, width, height, dIn if dOut is None else dOut, dStats),
               "jn_disparity_postfilter")


def filter_numpy(fp, maps, device=0):
    """Convenience for tests and scripts: host maps [n][H][W] int16 -> (filtered maps, stats [n][4]) through the device."""
    from .device import DeviceArray
    maps = np.ascontiguousarray(maps, np.int16)
    n, H, W = maps.shape
    d, s = DeviceArray.from_numpy(maps, device), DeviceArray((n, 4), np.uint32, device)
    disparity_postfilter(fp, n, d.ptr, W, H, None, s.ptr, device)
    out = d.numpy(), s.numpy()
    d.free(); s.free()
    return out


def attach(handle, slot, fp, dStats=None):
    """From now on every batch submitted on `slot` of an Sgm handle is filtered in place in its dDisp, ahead of the mono8 map, the scan and
    the attached tails; dStats [max_batch][4] uint32 (device) or None.  fp = None detaches.  No batch may be in flight on the slot.  The
    block matcher has no attach call."""
    from .sgm import Sgm
    if not isinstance(handle, Sgm):
        raise TypeError("attach() takes an Sgm handle; block-matching users call disparity_postfilter() on the slot's dDisp after Bm.wait()")
    _lib.check(_bind().jn_sgm_attach_postfilter(handle._h, slot, C.byref(fp) if fp is not None else None, dStats), "jn_sgm_attach_postfilter")

"""The mono8 node tail (include/jn_stereo.h: jn_disparity_to_u8, jn_build_valid_disp_lut, jn_obstacle_scan, jn_obstacle_scan_cloud,
jn_point_cloud) restated in numpy for any jn_scan_params: the checker of tests/test_gpu_rigs.py, itself pinned to
oracle/node_oracle.cpp under every rig of tests/rigs.py by tests/test_scan_def.py.  TEST INFRASTRUCTURE.  Every product, sum and quotient is
its own float64 numpy operation; the reprojection and the ground model are tests/costmap_def.py's, by import, and nothing is shared with
jackal_navigation_amd/."""
import numpy as np

from costmap_def import EMPTY, is_ground, reproject

META_INIT = (400.0, -400.0, 1e9, -500.0)


def to_u8(D):
    """convertTo(CV_8U): float32 rint (half to even), then saturation to 0..255.  Finite values and +-inf; NaN is not defined here."""
    d = np.asarray(D, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(d)                                                   # float32 in, float32 out
        r = np.where(r < np.float32(0), np.float32(0), np.where(r > np.float32(255), np.float32(255), r))
    return np.nan_to_num(r, nan=0.0).astype(np.uint8)


def valid_lut(sp, W, H):
    """[H][W][2] u8: the smallest d in 3..255 whose point reprojects (w != 0), has Z >= 0 and is not ground, 256 (none) stored as 0 like
    the reference's uchar; the second byte is 255."""
    first = np.full((H, W), 256, np.int64)
    for d in range(255, 2, -1):
        X, Y, Z, ok = reproject(sp, np.full((H, W), d, np.uint8))
        with np.errstate(all="ignore"):
            good = ok & ~(Z < 0.) & ~is_ground(sp, X, Z)
        first[good] = d
    lut = np.empty((H, W, 2), np.uint8)
    lut[..., 0] = (first & 255).astype(np.uint8)
    lut[..., 1] = 255
    return lut


def _scan(sp, X, Y, take):
    """bins [sp.bins], meta [4] and the smallest distance (in bins) of an obstacle pixel's bearing from a bin edge, as subpix_def.scan."""
    bins = np.full(sp.bins, EMPTY)
    meta = np.array(META_INIT)
    x, y = X[take], Y[take]
    with np.errstate(all="ignore"):
        th = np.arctan2(y, x)
        deg = th * 180. / sp.pi_approx
        r = np.sqrt(y * y + x * x)
        t = sp.bins * (sp.fov_deg / 2. + -deg) / sp.fov_deg
        kf = np.floor(t)
    if th.size:
        meta = np.array([th.min(), th.max(), r.min(), r.max()])
    inside = (kf >= 0) & (kf < sp.bins)
    np.minimum.at(bins, kf[inside].astype(np.int64), r[inside])
    edge = np.abs(t - np.rint(t))
    return bins, meta, (edge.min() if edge.size else 1.0)


def scan(sp, u8, lut):
    """The default flavour: the pixels with lut[0] <= d <= lut[1] whose w is not 0."""
    X, Y, Z, ok = reproject(sp, u8)
    d = u8.astype(np.int32)
    return _scan(sp, X, Y, ok & (d >= lut[..., 0].astype(np.int32)) & (d <= lut[..., 1].astype(np.int32)))


def scan_cloud(sp, u8):
    """The -g flavour: the pixels with d >= 2 whose w is not 0 and whose point is not ground."""
    X, Y, Z, ok = reproject(sp, u8)
    return _scan(sp, X, Y, ok & (u8 >= 2) & ~is_ground(sp, X, Z))


def cloud(sp, u8):
    """float32 xyz [count][3] of the pixels with d >= 2, i outer / j inner; w = 0 gives (0, 0, 0)."""
    X, Y, Z, ok = reproject(sp, u8)
    P = np.stack([np.where(ok, X, 0.), np.where(ok, Y, 0.), np.where(ok, Z, 0.)], axis=-1)       # [H][W][3]
    with np.errstate(all="ignore"):
        return P.transpose(1, 0, 2)[(u8 >= 2).T].astype(np.float32)


def cloud_w_nonzero(sp, u8):
    """bool [count]: the rows of cloud() whose w is not 0 (oracle/node_oracle.cpp leaves the others out: its one stated divergence)."""
    return reproject(sp, u8)[3].T[(u8 >= 2).T]

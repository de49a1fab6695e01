"""The scalar definition of the sub-pixel navigation tail (include/jn_subpix.h) restated in numpy: the checker of tests/test_gpu_subpix.py
and tests/test_subpix_api.py.  TEST INFRASTRUCTURE.  Every product, sum and quotient is its own float64 numpy operation, in the order of
the header; the reprojection, the ground model and the grid classification are tests/costmap_def.py's, by import."""
import numpy as np

import costmap_def as cd

EMPTY = cd.EMPTY
F32, I16, I16_SUB = 0, 1, 2
MAX_Q = 16 * 4096
META_INIT = (400.0, -400.0, 1e9, -500.0)


def to_q(maps, fmt, min_q=32):
    """-> (q int64, valid bool), the shape of maps."""
    if fmt == F32:
        d = np.asarray(maps, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.rint(np.float32(16) * d)                              # float32; numpy's rint rounds half to even
            valid = np.isfinite(d) & (t >= np.float32(min_q)) & (t <= np.float32(MAX_Q))
        q = np.where(valid, t, 0).astype(np.int64)
    else:
        q = np.asarray(maps, np.int16).astype(np.int64) * (16 if fmt == I16 else 1)
        valid = (q >= min_q) & (q <= MAX_Q)
    return q, valid


def reproject(sp, q):
    """q [H][W] -> X, Y, Z float64 and the mask of pixels whose homogeneous w is not 0: costmap_def's expression with d = q / 16.0."""
    return cd.reproject(sp, np.asarray(q, np.float64) / 16.0)


def obstacles(sp, q, valid):
    """-> X, Y, Z, take: the obstacle mask of one map."""
    X, Y, Z, ok = reproject(sp, q)
    return X, Y, Z, valid & ok & ~cd.is_ground(sp, X, Z)


def scan(sp, q, valid):
    """bins [sp.bins], meta [4], and per bin the margin (in bins) by which the nearest obstacle pixel of the frame misses a bin edge —
    a device atan2 one ulp away moves only pixels within that margin."""
    X, Y, Z, take = obstacles(sp, q, valid)
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
    k = kf[inside].astype(np.int64)
    np.minimum.at(bins, k, r[inside])
    edge = np.abs(t - np.rint(t))
    return bins, meta, (edge.min() if edge.size else 1.0)


def hits(sp, cp, q, valid):
    """hits [cells_y][cells_x] u16 of one map (jn_costmap.h's "cell" and "hits" over the obstacle pixels)."""
    X, Y, Z, take = obstacles(sp, q, valid)
    with np.errstate(all="ignore"):
        fx = np.floor((X - cp.origin_x) / cp.resolution)
        fy = np.floor((Y - cp.origin_y) / cp.resolution)
        take = take & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (fx >= 0) & (fx < cp.cells_x) & (fy >= 0) & (fy < cp.cells_y)
    c = np.bincount(fy[take].astype(np.int64) * cp.cells_x + fx[take].astype(np.int64), minlength=cp.cells_x * cp.cells_y)
    return np.minimum(c, 65535).astype(np.uint16).reshape(cp.cells_y, cp.cells_x)


classify = cd.classify                 # grid from hits and bins: jn_costmap.h's "grid", unchanged


def cloud(sp, q, valid):
    """float32 xyz [count][3] of the valid pixels, i outer / j inner; w = 0 gives (0, 0, 0)."""
    X, Y, Z, ok = reproject(sp, q)
    P = np.stack([np.where(ok, X, 0.), np.where(ok, Y, 0.), np.where(ok, Z, 0.)], axis=-1)       # [H][W][3]
    with np.errstate(all="ignore"):
        return P.transpose(1, 0, 2)[valid.T].astype(np.float32)


def wall_q(sp, W, H, distance):
    """The true disparity, in 1/16 pixel (rounded to the nearest), of a fronto-parallel wall `distance` metres along the optical axis:
    camera z = Q[2][3] / (Q[3][2] d + Q[3][3]) solved for d."""
    Q = list(sp.Q)
    d = (Q[11] / distance - Q[15]) / Q[14]
    return np.full((H, W), int(np.rint(16.0 * d)), np.int64), d

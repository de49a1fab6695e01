"""The scalar definition of the obstacle costmap (include/jn_costmap.h) restated in numpy: the checker of tests/test_gpu_costmap.py.
TEST INFRASTRUCTURE.  Every product, sum and quotient is its own float64 numpy operation (numpy evaluates `a + b * c` as two rounded
steps), exactly the expressions of the header."""
import math

import numpy as np

EMPTY = 1e9                      # JN_SCAN_EMPTY


def reproject(sp, disp):
    """disp [H][W] u8 -> X, Y, Z [H][W] float64 in the robot frame and the mask of pixels whose homogeneous w is not 0."""
    H, W = disp.shape
    V0 = np.broadcast_to((np.arange(W, dtype=np.int64)[None, :] + sp.crop_offset_x).astype(np.float64), (H, W))
    V1 = np.broadcast_to((np.arange(H, dtype=np.int64)[:, None] + sp.crop_offset_y).astype(np.float64), (H, W))
    V2 = disp.astype(np.float64)
    Q, XR, XT = list(sp.Q), list(sp.XR), list(sp.XT)
    pos = []
    for r in range(4):
        a = Q[4 * r] * V0
        a = a + Q[4 * r + 1] * V1
        a = a + Q[4 * r + 2] * V2
        a = a + Q[4 * r + 3]
        pos.append(a)
    ok = pos[3] != 0.0
    with np.errstate(all="ignore"):
        cam = [pos[k] / pos[3] for k in range(3)]
        out = []
        for r in range(3):
            a = XR[3 * r] * cam[0]
            a = a + XR[3 * r + 1] * cam[1]
            a = a + XR[3 * r + 2] * cam[2]
            out.append(a + XT[r])
    return out[0], out[1], out[2], ok


def is_ground(sp, X, Z):
    with np.errstate(all="ignore"):
        return np.where(X < sp.gp_dist_thresh, Z < sp.gp_height_thresh,
                        Z < sp.gp_height_thresh + math.tan(sp.gp_angle_thresh) * (X - sp.gp_dist_thresh))


def obstacle_cells(sp, cp, disp, lut):
    """Flat cell index iy * cells_x + ix of every obstacle pixel of one map that lands inside the grid."""
    X, Y, Z, ok = reproject(sp, disp)
    d = disp.astype(np.int32)
    if cp.from_cloud:
        take = ok & (d >= 2) & ~is_ground(sp, X, Z)
    else:
        take = ok & (d >= lut[..., 0].astype(np.int32)) & (d <= lut[..., 1].astype(np.int32))
    with np.errstate(all="ignore"):
        fx = np.floor((X - cp.origin_x) / cp.resolution)
        fy = np.floor((Y - cp.origin_y) / cp.resolution)
        take = take & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (fx >= 0) & (fx < cp.cells_x) & (fy >= 0) & (fy < cp.cells_y)
    return fy[take].astype(np.int64) * cp.cells_x + fx[take].astype(np.int64)


def hits(sp, cp, disp, lut):
    """hits [cells_y][cells_x] u16 of one map."""
    c = np.bincount(obstacle_cells(sp, cp, disp, lut), minlength=cp.cells_x * cp.cells_y)
    return np.minimum(c, 65535).astype(np.uint16).reshape(cp.cells_y, cp.cells_x)


def classify(sp, cp, h, bins, margin=1e-9):
    """(grid [cells_y][cells_x] int8, decided): grid from hits `h` and one frame's bins (None: no cell is free); `decided` is False where
    the free / unknown decision sits within `margin` of a bin edge or of the range threshold (one atan2 / sqrt apart: not compared)."""
    cy, cx = cp.cells_y, cp.cells_x
    grid = np.full((cy, cx), -1, np.int8)
    decided = np.ones((cy, cx), bool)
    if bins is not None:
        xc = np.broadcast_to((cp.origin_x + (np.arange(cx, dtype=np.float64) + 0.5) * cp.resolution)[None, :], (cy, cx))
        yc = np.broadcast_to((cp.origin_y + (np.arange(cy, dtype=np.float64) + 0.5) * cp.resolution)[:, None], (cy, cx))
        th = np.arctan2(yc, xc)
        deg = th * 180. / sp.pi_approx
        t = sp.bins * (sp.fov_deg / 2. + -deg) / sp.fov_deg
        kf = np.floor(t)
        inside = (kf >= 0) & (kf < sp.bins)
        k = np.where(inside, kf, 0).astype(np.int64)
        b = np.asarray(bins, np.float64)[k]
        r = np.sqrt(yc * yc + xc * xc) + cp.resolution
        free = inside & (b < EMPTY - 1) & (r <= b)
        grid[free] = 0
        decided = (np.abs(t - np.rint(t)) > margin) & (np.abs(r - b) > margin)
    occ = h >= cp.min_hits
    grid[occ] = 100
    decided = decided | occ
    return grid, decided

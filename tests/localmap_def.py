"""The scalar definition of the odometry-fused local obstacle map (include/jn_localmap.h) restated in numpy: the checker of
tests/test_gpu_localmap.py and tests/test_localmap_api.py.  TEST INFRASTRUCTURE.  Every product, sum and quotient is its own float64 numpy
operation, in the order of the header; the conversion to 1/16 pixel and the reprojection are tests/subpix_def.py's, the ground model is
tests/costmap_def.py's, by import."""
import math

import numpy as np

import costmap_def as cd
import subpix_def as sd

F32, I16, I16_SUB = sd.F32, sd.I16, sd.I16_SUB


def centre_on(p, x, y):
    """jn_localmap.h "recentre": the global index of cell (0, 0) of the window centred on (x, y)."""
    return (int(math.floor(x / p.resolution)) - p.cells_x // 2, int(math.floor(y / p.resolution)) - p.cells_y // 2)


def counts(sp, p, g0, pose, m):
    """One map `m` [H][W] in p.format seen from pose (x, y, theta) -> (obst, floor) [cells_y][cells_x] u16 in the window at g0."""
    q, valid = sd.to_q(m, p.format, p.min_q)
    X, Y, Z, ok = sd.reproject(sp, q)
    ground = cd.is_ground(sp, X, Z)
    x, y, theta = pose
    c, s = math.cos(theta), math.sin(theta)
    ox, oy = float(g0[0]) * p.resolution, float(g0[1]) * p.resolution
    with np.errstate(all="ignore"):
        Xw = (c * X - s * Y) + x
        Yw = (s * X + c * Y) + y
        fx = np.floor((Xw - ox) / p.resolution)
        fy = np.floor((Yw - oy) / p.resolution)
        inside = valid & ok & np.isfinite(Xw) & np.isfinite(Yw) & np.isfinite(Z) & (fx >= 0) & (fx < p.cells_x) & (fy >= 0) & (fy < p.cells_y)
    out = []
    for take in (inside & ~ground, inside & ground):
        k = np.bincount(fy[take].astype(np.int64) * p.cells_x + fx[take].astype(np.int64), minlength=p.cells_x * p.cells_y)
        out.append(np.minimum(k, 65535).astype(np.uint16).reshape(p.cells_y, p.cells_x))
    return out[0], out[1]


def fuse(p, L, obst, floor):
    """One frame's evidence applied to L (int16 [cells_y][cells_x]) -> the new L."""
    l = L.astype(np.int64)
    hit = obst >= p.min_hits
    miss = ~hit & (floor >= p.min_floor)
    l = np.where(hit, np.minimum(l + p.l_hit, p.l_max), l)
    l = np.where(miss, np.maximum(l - p.l_miss, p.l_min), l)
    return l.astype(np.int16)


def grid(p, L):
    g = np.full(L.shape, -1, np.int8)
    g[L >= p.occ_thresh] = 100
    g[L <= p.free_thresh] = 0
    return g


def shift(p, L, g_old, g_new):
    """L of the window at g_old -> L of the window at g_new: the overlap kept, entering cells 0."""
    out = np.zeros_like(L)
    dx, dy = g_new[0] - g_old[0], g_new[1] - g_old[1]
    for iy in range(max(0, -dy), min(p.cells_y, p.cells_y - dy)):
        x0, x1 = max(0, -dx), min(p.cells_x, p.cells_x - dx)
        if x1 > x0:
            out[iy, x0:x1] = L[iy + dy, x0 + dx:x1 + dx]
    return out


class Map:
    """The handle's life restated: reset state at construction, update / recenter / reset as the C ABI's."""

    def __init__(self, p):
        self.p = p
        self.reset()

    def reset(self):
        self.L = np.zeros((self.p.cells_y, self.p.cells_x), np.int16)
        self.g0 = centre_on(self.p, 0.0, 0.0)

    def recenter(self, x, y):
        g = centre_on(self.p, x, y)
        self.L = shift(self.p, self.L, self.g0, g)
        self.g0 = g

    def update(self, sp, poses, maps):
        """-> (obst, floor) [n][cells_y][cells_x] u16 of the frames; L advanced through them in index order."""
        O, F = [], []
        for pose, m in zip(poses, maps):
            o, f = counts(sp, self.p, self.g0, pose, m)
            self.L = fuse(self.p, self.L, o, f)
            O.append(o); F.append(f)
        return np.stack(O), np.stack(F)

    def grid(self):
        return grid(self.p, self.L)

"""The scalar definition of the local planner (include/jn_plan.h) restated in numpy / plain Python: the checker of
tests/test_gpu_plan.py and tests/test_plan_api.py.  TEST INFRASTRUCTURE, written from the header.  clearance() is the LITERAL definition —
for every cell the minimum over all obstacle cells, no separable shortcut; templates(), rollout() and choose() do every product, sum,
quotient and square root as its own Python float operation, in the order of the header, with math.sin / math.cos (the C library's)."""
import math

import numpy as np

FAR = 65535
OK, BLOCKED = 0, 1
RECORD_DTYPE = np.dtype([("t_end", np.int32), ("t_hit", np.int32), ("min_d2", np.int32), ("last_cell", np.int32)])


def obstacles(grid, unknown_is_obstacle):
    g = np.asarray(grid, np.int8)
    return (g == 100) | ((g == -1) if unknown_is_obstacle else False)


def _by_obstacle(obst, radius):
    """For every cell the minimum of dx^2 + dy^2 over ALL obstacle cells, one obstacle after the other (in chunks, to bound memory)."""
    cy, cx = obst.shape
    oy, ox = np.nonzero(obst)
    best = np.full((cy, cx), np.iinfo(np.int64).max, np.int64)
    ys = np.arange(cy, dtype=np.int64)[:, None, None]
    xs = np.arange(cx, dtype=np.int64)[None, :, None]
    chunk = max(1, (1 << 23) // (cy * cx))
    for k in range(0, len(oy), chunk):
        dy = ys - oy[None, None, k:k + chunk]
        dx = xs - ox[None, None, k:k + chunk]
        best = np.minimum(best, (dx * dx + dy * dy).min(axis=2))
    return np.where(best <= radius * radius, best, FAR).astype(np.uint16)


def _by_offset(obst, radius):
    """The same minimum with the loops exchanged: every offset (dx, dy) of the disk in the order of dx^2 + dy^2; a cell takes the value of
    the first offset at which it meets an obstacle cell.  Stops when no cell is left (a dense grid is done after a few offsets)."""
    cy, cx = obst.shape
    r = np.arange(-radius, radius + 1)
    DY, DX = np.meshgrid(r, r, indexing="ij")
    D = DX * DX + DY * DY
    keep = (D <= radius * radius) & (np.abs(DX) < cx) & (np.abs(DY) < cy)
    order = np.argsort(D[keep], kind="stable")
    out = np.full((cy, cx), FAR, np.uint16)
    left = cy * cx
    for dx, dy, d in zip(DX[keep][order].tolist(), DY[keep][order].tolist(), D[keep][order].tolist()):
        # cells (y, x) with (y + dy, x + dx) inside the grid
        y0, y1, x0, x1 = max(0, -dy), min(cy, cy - dy), max(0, -dx), min(cx, cx - dx)
        view = out[y0:y1, x0:x1]
        take = obst[y0 + dy:y1 + dy, x0 + dx:x1 + dx] & (view == FAR)
        k = int(take.sum())
        if k:
            view[take] = d
            left -= k
            if left == 0:
                break
    return out


def clearance(grid, radius, unknown_is_obstacle=0):
    """grid [cells_y][cells_x] int8 -> d2 [cells_y][cells_x] u16, the literal definition: for each cell the minimum over the obstacle cells
    within the radius.  Brute force either obstacle by obstacle or offset by offset, whichever loop is shorter; no separable pass."""
    g = np.asarray(grid, np.int8)
    assert g.ndim == 2 and 1 <= radius <= 255
    obst = obstacles(g, unknown_is_obstacle)
    if int(obst.sum()) <= 3 * radius * radius:
        return _by_obstacle(obst, radius)
    return _by_offset(obst, radius)


def clearance_batch(grids, radius, unknown_is_obstacle=0):
    return np.stack([clearance(g, radius, unknown_is_obstacle) for g in grids])


def candidate(p, k):
    iv, iw = divmod(k, p.n_w)
    m = (p.n_w - 1) // 2
    v = (p.v_max * float(iv + 1)) / float(p.n_v)
    w = 0.0 if m == 0 else (p.w_max * float(iw - m)) / float(m)
    return v, w


def point(p, v, w, s):
    t = (p.horizon * float(s + 1)) / float(p.steps)
    if w == 0.0:
        return v * t, 0.0
    r = v / w
    a = w * t
    return r * math.sin(a), r * (1.0 - math.cos(a))


def templates(p):
    """-> (v [K], w [K], xy [K][steps][2]) float64."""
    K = p.n_v * p.n_w
    v, w, xy = np.empty(K), np.empty(K), np.empty((K, p.steps, 2))
    for k in range(K):
        v[k], w[k] = candidate(p, k)
        for s in range(p.steps):
            xy[k, s] = point(p, float(v[k]), float(w[k]), s)
    return v, w, xy


def r2_of(p, resolution):
    q = p.robot_radius / resolution
    return int(math.floor(q * q))


def cell_of(Xw, Yw, origin, resolution, cells_x, cells_y):
    """jn_costmap.h's "cell" -> index or -1."""
    if not (math.isfinite(Xw) and math.isfinite(Yw)):
        return -1
    fx = math.floor((Xw - origin[0]) / resolution)
    fy = math.floor((Yw - origin[1]) / resolution)
    if 0 <= fx < cells_x and 0 <= fy < cells_y:
        return int(fy) * cells_x + int(fx)
    return -1


def rollout(p, resolution, d2, origin, pose):
    """One frame: d2 [cells_y][cells_x] u16, the grid's origin (x, y), pose (x, y, theta) -> records RECORD_DTYPE [K]."""
    cy, cx = d2.shape
    flat = np.asarray(d2).reshape(-1)
    x, y, theta = (float(t) for t in pose)
    c, s = math.cos(theta), math.sin(theta)
    r2, T = r2_of(p, resolution), p.steps
    K = p.n_v * p.n_w
    rec = np.empty(K, RECORD_DTYPE)
    for k in range(K):
        v, w = candidate(p, k)
        t_end, t_hit, mn, last = T, T, FAR, -1
        for st in range(T):
            xt, yt = point(p, v, w, st)
            Xw = (c * xt - s * yt) + x
            Yw = (s * xt + c * yt) + y
            cell = cell_of(Xw, Yw, origin, resolution, cx, cy)
            if cell < 0:
                t_end = st
                break
            d = int(flat[cell])
            if d <= r2:
                t_hit = st
                break
            mn = min(mn, d)
            last = cell
        rec[k] = (t_end, t_hit, mn, last)
    return rec


def choose(p, resolution, rec, pose, goal):
    """-> (v, w, candidate, status)."""
    x, y, theta = (float(t) for t in pose)
    c, s = math.cos(theta), math.sin(theta)
    T = p.steps
    best, out = None, (0.0, 0.0, -1, BLOCKED)
    for k in range(p.n_v * p.n_w):
        t_end, t_hit, min_d2 = int(rec[k]["t_end"]), int(rec[k]["t_hit"]), int(rec[k]["min_d2"])
        if t_hit != T or t_end < 1:
            continue
        v, w = candidate(p, k)
        xt, yt = point(p, v, w, t_end - 1)
        ex = (c * xt - s * yt) + x
        ey = (s * xt + c * yt) + y
        dx = ex - float(goal[0])
        dy = ey - float(goal[1])
        dist = math.sqrt(dx * dx + dy * dy)
        clear = min(math.sqrt(float(min_d2)) * resolution, p.clear_cap)
        score = (p.w_goal * dist - p.w_clear * clear) - p.w_speed * v
        if best is None or score < best:
            best, out = score, (v, w, k, OK)
    return out

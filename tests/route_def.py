"""The scalar definition of the cost-to-go field (include/jn_route.h) restated in plain Python and numpy: the checker of
tests/test_gpu_route.py and tests/test_route_api.py.  TEST INFRASTRUCTURE, written from the header.  field() is Dijkstra with a heap over
the 8 moves in the header's order — no sweeps, no tiles, nothing of the kernels' schedule; goal_cell(), gather(), choose() and trace() do
what the header says in its order, choose() with every product and quotient as its own Python float operation, reusing plan_def where
the two definitions are the same."""
import heapq
import math

import numpy as np

import plan_def as pd

UNREACHED = 65535
OK, NO_ROUTE = 0, 1
MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))      # (dx, dy), the fixed order
WEIGHTS = (5, 5, 5, 5, 7, 7, 7, 7)


class Params:
    """jn_route_params with its defaults."""

    def __init__(self, near_radius=10, near_penalty=3, goal_radius=2, reserved=0):
        self.near_radius, self.near_penalty, self.goal_radius, self.reserved = near_radius, near_penalty, goal_radius, reserved


def goal_cell(resolution, cells_x, cells_y, origin, goal):
    """-> (ix, iy): jn_costmap.h's cell arithmetic, each index clamped onto the grid."""
    out = []
    for X, o, cells in ((float(goal[0]), float(origin[0]), cells_x), (float(goal[1]), float(origin[1]), cells_y)):
        assert math.isfinite(X)
        q = (X - o) / resolution
        f = math.floor(q) if math.isfinite(q) else q
        out.append(cells - 1 if f >= cells - 1 else int(f) if f >= 0 else 0)
    return tuple(out)


def seeds_of(d2, r2, rp, goal):
    """-> bool [cells_y][cells_x]: the passable cells within goal_radius of the goal cell (gx, gy)."""
    cy, cx = d2.shape
    ys, xs = np.mgrid[0:cy, 0:cx]
    return (d2.astype(np.int64) > r2) & ((xs - goal[0]) ** 2 + (ys - goal[1]) ** 2 <= rp.goal_radius ** 2)


def field(d2, r2, rp, goal):
    """One frame: d2 [cells_y][cells_x] u16, the goal cell (gx, gy) -> (g [cells_y][cells_x] u16, the number of seeds)."""
    d2 = np.asarray(d2)
    cy, cx = d2.shape
    passable = (d2.astype(np.int64) > r2)
    pen = np.where(d2.astype(np.int64) <= rp.near_radius ** 2, rp.near_penalty, 0).tolist()
    ok = passable.tolist()
    seeds = seeds_of(d2, r2, rp, goal)
    g = [[UNREACHED] * cx for _ in range(cy)]
    heap = []
    for y, x in zip(*np.nonzero(seeds)):
        g[int(y)][int(x)] = 0
        heap.append((0, int(x), int(y)))
    heapq.heapify(heap)
    while heap:
        v, x, y = heapq.heappop(heap)
        if v != g[y][x]:
            continue
        # the cells c that may step INTO (x, y): c's cost is w + pen(x, y) + g(x, y)
        base = v + pen[y][x]
        for (dx, dy), w in zip(MOVES, WEIGHTS):
            cx_, cy_ = x - dx, y - dy
            if 0 <= cx_ < cx and 0 <= cy_ < cy and ok[cy_][cx_]:
                t = base + w
                if t <= 65534 and t < g[cy_][cx_]:
                    g[cy_][cx_] = t
                    heapq.heappush(heap, (t, cx_, cy_))
    return np.array(g, np.uint16).reshape(cy, cx), int(seeds.sum())


def field_batch(d2s, r2, rp, goals):
    out = [field(d2s[f], r2, rp, goals[f]) for f in range(len(d2s))]
    return np.stack([o[0] for o in out]), [o[1] for o in out]


def gather(g, rec):
    """g [cells_y][cells_x], rec RECORD_DTYPE [K] -> togo u16 [K]."""
    flat = np.asarray(g).reshape(-1)
    return np.array([UNREACHED if int(c) < 0 else int(flat[int(c)]) for c in rec["last_cell"]], np.uint16)


def choose(p, resolution, rec, togo):
    """-> (v, w, candidate, status): plan_def.choose with the header's two changes."""
    T = p.steps
    best, out = None, (0.0, 0.0, -1, pd.BLOCKED)
    for k in range(p.n_v * p.n_w):
        t_end, t_hit, min_d2 = int(rec[k]["t_end"]), int(rec[k]["t_hit"]), int(rec[k]["min_d2"])
        if t_hit != T or t_end < 1 or int(togo[k]) == UNREACHED:
            continue
        v, w = pd.candidate(p, k)
        dist = (float(int(togo[k])) * resolution) / 5.0
        clear = min(math.sqrt(float(min_d2)) * resolution, p.clear_cap)
        score = (p.w_goal * dist - p.w_clear * clear) - p.w_speed * v
        if best is None or score < best:
            best, out = score, (v, w, k, pd.OK)
    return out


def trace(g, d2, r2, rp, start):
    """-> (cells, status): the indices iy * cells_x + ix from the start cell (x, y) to a seed."""
    g, d2 = np.asarray(g), np.asarray(d2)
    cy, cx = g.shape
    x, y = start
    if not (0 <= x < cx and 0 <= y < cy) or int(g[y, x]) == UNREACHED:
        return [], NO_ROUTE
    cells = [y * cx + x]
    while int(g[y, x]) != 0:
        for (dx, dy), w in zip(MOVES, WEIGHTS):
            mx, my = x + dx, y + dy
            if not (0 <= mx < cx and 0 <= my < cy) or int(d2[my, mx]) <= r2 or int(g[my, mx]) == UNREACHED:
                continue
            if w + (rp.near_penalty if int(d2[my, mx]) <= rp.near_radius ** 2 else 0) + int(g[my, mx]) == int(g[y, x]):
                x, y = mx, my
                break
        else:
            raise AssertionError("g is not the field of these inputs at (%d, %d)" % (x, y))
        cells.append(y * cx + x)
    return cells, OK


def path_cost(cells, d2, rp):
    """The sum of w + pen over the steps of a traced path."""
    d2 = np.asarray(d2)
    cx = d2.shape[1]
    total = 0
    for a, b in zip(cells[:-1], cells[1:]):
        dx, dy = b % cx - a % cx, b // cx - a // cx
        assert max(abs(dx), abs(dy)) == 1
        total += (5 if dx == 0 or dy == 0 else 7) + (rp.near_penalty if int(d2[b // cx, b % cx]) <= rp.near_radius ** 2 else 0)
    return total


# ---- a robot driven by either chooser (the dead-end scenario of both test files) ----

def advance(pose, v, w, dt):
    """plan_def.point's kinematics over dt from pose (x, y, theta)."""
    x, y, th = pose
    if w == 0.0:
        xt, yt = v * dt, 0.0
    else:
        r = v / w
        a = w * dt
        xt, yt = r * math.sin(a), r * (1.0 - math.cos(a))
    c, s = math.cos(th), math.sin(th)
    return ((c * xt - s * yt) + x, (s * xt + c * yt) + y, th + w * dt)

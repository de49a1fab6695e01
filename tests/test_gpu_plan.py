"""The local planner (include/jn_plan.h) on the GPU against its scalar definition (tests/plan_def.py), everything bit for bit: the
clearance field, the rollout records and the chosen command; behaviour on an empty map, a wall and a closed box; end to end behind the
local map and behind the sub-pixel costmap.

Kernel forms: k_clearance has ONE form for every grid size and radius (the halo is staged as bits, so it fits the LDS up to radius 255);
every case below runs it.  What varies inside it is covered by the sizes: grids narrower than a wave and than the workgroup (1, 37, 53
columns), a last band that is partly outside the grid (37, 53, 1 rows), halos that lie wholly outside the grid (radius 255 on small
grids) and wholly inside it (radius 1 .. 20 on 512 rows), 1 to 17 bit words per column."""
import ctypes as C
import math

import numpy as np
import pytest

import localmap_def as ld
import plan_def as pd
import subpix_def as sd

pytestmark = pytest.mark.gpu

POISON = 0xABCD


def gpu_clearance(grids, R, unk):
    """n grids through the device-pointer form of plan.clearance, the output poisoned beforehand."""
    from jackal_navigation_amd import plan
    from jackal_navigation_amd.device import DeviceArray
    n, cy, cx = grids.shape
    dG = DeviceArray.from_numpy(grids)
    dD = DeviceArray.from_numpy(np.full((n, cy, cx), POISON, np.uint16))
    plan.clearance(dG.ptr, R, unk, n, cx, cy, dD.ptr)
    out = dD.numpy()
    dG.free(); dD.free()
    return out


def random_grids(rng, n, cy, cx, dens):
    """Frame f has obstacle density dens[f % len(dens)] (0: exactly one obstacle cell), blocks of unknown cells of up to 30 x 30, a few
    free (0) cells on top of unknown ones, values that are not obstacles (1 .. 99)."""
    g = np.zeros((n, cy, cx), np.int8)
    for f in range(n):
        d = dens[f % len(dens)]
        for _ in range(3):
            y0, x0 = int(rng.integers(0, cy)), int(rng.integers(0, cx))
            g[f, y0:y0 + int(rng.integers(1, 31)), x0:x0 + int(rng.integers(1, 31))] = -1
        g[f][rng.random((cy, cx)) < 0.02] = rng.integers(1, 100)
        if d == 0:
            g[f, int(rng.integers(0, cy)), int(rng.integers(0, cx))] = 100
        else:
            g[f][rng.random((cy, cx)) < d] = 100
    return g


def check_clearance(grids, R, what):
    for unk in (0, 1):
        got = gpu_clearance(grids, R, unk)
        assert got.dtype == np.uint16 and got.shape == grids.shape
        for f in range(grids.shape[0]):
            want = pd.clearance(grids[f], R, unk)
            assert np.array_equal(got[f], want), (what, R, unk, f, int((got[f] != want).sum()))


CLEARANCE_CASES = [
    # cy, cx, n, radii, densities
    (1, 1, 1, (1, 255), (1.0,)),
    (1, 1, 3, (2,), (0, 0.0001, 1.0)),
    (1, 512, 3, (1, 20, 255), (0, 0.01, 0.3)),
    (512, 1, 3, (2, 64, 255), (0, 0.01, 0.3)),
    (53, 37, 32, (1, 2, 20, 64, 255), (0, 0.001, 0.01, 0.1, 0.5, 0.95)),
    (37, 53, 1, (20,), (0.02,)),
    (128, 128, 3, (2, 20, 64), (0, 0.002, 0.3)),
    (128, 128, 32, (20,), (0, 0.0005, 0.005, 0.05, 0.5)),
    (256, 256, 3, (1, 20, 255), (0, 0.001, 0.3)),
    (512, 512, 1, (20, 255), (0.0006,)),
    (512, 512, 1, (2, 64), (0.3,)),
    (512, 512, 3, (1,), (0, 0.01, 0.6)),
]


@pytest.mark.parametrize("cy,cx,n,radii,dens", CLEARANCE_CASES, ids=["%dx%dx%d" % (c[2], c[0], c[1]) for c in CLEARANCE_CASES])
def test_clearance_equals_the_definition(jn, cy, cx, n, radii, dens):
    rng = np.random.default_rng(cy * 1000 + cx + n)
    grids = random_grids(rng, n, cy, cx, dens)
    for R in radii:
        check_clearance(grids, R, (cy, cx, n))


@pytest.mark.parametrize("cy,cx", [(128, 128), (53, 37), (512, 512), (1, 512), (512, 1)])
def test_clearance_with_obstacles_on_every_border_and_corner(jn, cy, cx):
    corners = np.zeros((cy, cx), np.int8)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 100
    one = [np.zeros((cy, cx), np.int8) for _ in range(4)]
    one[0][0, 0] = 100; one[1][0, -1] = 100; one[2][-1, 0] = 100; one[3][-1, -1] = 100
    frames = [corners] + one
    if cy * cx <= 128 * 128:
        border = np.zeros((cy, cx), np.int8)
        border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = 100
        edges = [np.zeros((cy, cx), np.int8) for _ in range(4)]
        edges[0][0, :] = 100; edges[1][-1, :] = 100; edges[2][:, 0] = -1; edges[3][:, -1] = -1
        frames += [border] + edges
    grids = np.stack(frames)
    for R in (1, 20, 255):
        check_clearance(grids, R, ("border", cy, cx))


def test_clearance_empty_full_repeatable_and_invalid_calls(jn):
    from jackal_navigation_amd import plan, _lib
    from jackal_navigation_amd.device import DeviceArray
    g = np.zeros((2, 100, 70), np.int8)
    g[1] = 100
    for R in (1, 64, 255):
        out = gpu_clearance(g, R, 0)
        assert (out[0] == pd.FAR).all() and (out[1] == 0).all()
    u = np.full((1, 64, 64), -1, np.int8)
    assert (gpu_clearance(u, 9, 0) == pd.FAR).all() and (gpu_clearance(u, 9, 1) == 0).all()
    rng = np.random.default_rng(2)
    r = random_grids(rng, 2, 200, 300, (0.01,))
    a, b = gpu_clearance(r, 33, 1), gpu_clearance(r, 33, 1)
    assert np.array_equal(a, b)
    # the numpy form of the same call: a 2-D grid gives a 2-D field
    assert np.array_equal(plan.clearance(r[0], 33, 1), a[0]) and np.array_equal(plan.clearance(r, 33, 1), a)
    # an invalid call leaves the output alone
    dG = DeviceArray.from_numpy(r); dD = DeviceArray.from_numpy(np.full(r.shape, POISON, np.uint16))
    for bad in (dict(R=0), dict(R=256), dict(unk=2), dict(n=0), dict(cx=0), dict(cy=513)):
        kw = dict(R=5, unk=0, n=2, cx=300, cy=200); kw.update(bad)
        with pytest.raises(_lib.JnError) as e:
            plan.clearance(dG.ptr, kw["R"], kw["unk"], kw["n"], kw["cx"], kw["cy"], dD.ptr)
        assert e.value.status == _lib.JN_ERR_INVALID
    assert (dD.numpy() == POISON).all()


# ---- rollouts ----

def gpu_plan(p, res, fields, origin, poses, goals):
    """-> (records [n][K], [(v, w, candidate, status)]) from jn_plan_command on device fields; evaluate alone must give the same records."""
    from jackal_navigation_amd import plan
    from jackal_navigation_amd.device import DeviceArray
    n, cy, cx = fields.shape
    dF = DeviceArray.from_numpy(fields)
    with plan.Plan(p, res, cx, cy, max_batch=n) as pl:
        cmds, rec = pl.command(dF.ptr, origin, poses, goals, with_records=True)
        rec2 = pl.evaluate(dF.ptr, origin, poses)
        assert np.array_equal(rec, rec2)
        assert [(c.v, c.w, c.candidate, c.status) for c in pl.command(dF.ptr, origin, poses, goals)] == [(c.v, c.w, c.candidate, c.status) for c in cmds]
    dF.free()
    return rec, [(c.v, c.w, c.candidate, c.status) for c in cmds]


def check_plan(p, res, fields, origin, poses, goals, what=None):
    rec, cmds = gpu_plan(p, res, fields, origin, poses, goals)
    for f in range(len(poses)):
        want = pd.rollout(p, res, fields[f], origin, poses[f])
        assert np.array_equal(rec[f], want), (what, f, poses[f], np.nonzero(rec[f] != want)[0][:5])
        wc = pd.choose(p, res, want, poses[f], goals[f])
        assert cmds[f][2:] == wc[2:], (what, f, cmds[f], wc)
        assert np.array_equal(np.array(cmds[f][:2]).view(np.uint64), np.array(wc[:2]).view(np.uint64)), (what, f)
    return rec, cmds


def window_poses(rng, res, cx, cy, origin, n):
    """Poses inside the window, near each edge (within a cell of it, inside and outside) and far outside; theta over a full turn."""
    x0, y0, x1, y1 = origin[0], origin[1], origin[0] + cx * res, origin[1] + cy * res
    out = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            x, y = rng.uniform(x0, x1), rng.uniform(y0, y1)
        elif kind == 1:
            x, y = rng.choice([x0, x1]) + rng.uniform(-res, res), rng.uniform(y0, y1)
        elif kind == 2:
            x, y = rng.uniform(x0, x1), rng.choice([y0, y1]) + rng.uniform(-res, res)
        else:
            x, y = x1 + rng.uniform(0.1, 3.0), y0 - rng.uniform(0.1, 3.0)
        out.append((float(x), float(y), float(-math.pi + 2 * math.pi * k / n + rng.uniform(-0.05, 0.05))))
    return out


@pytest.mark.parametrize("cy,cx,res,R,dens", [(256, 256, 0.05, 20, 0.01), (53, 37, 0.1, 64, 0.01), (128, 128, 0.05, 20, 0.01), (1, 1, 2.0, 3, 0),
                                              (512, 512, 0.03, 20, 0.005)])
def test_records_and_commands_equal_the_definition(jn, cy, cx, res, R, dens):
    from jackal_navigation_amd import plan
    rng = np.random.default_rng(7 * cy + cx)
    n = 24
    grids = random_grids(rng, 3, cy, cx, (dens,))
    fields = gpu_clearance(grids, R, 0)[np.arange(n) % 3]                  # the device's own fields, checked above
    origin = (-cx * res / 2 + 0.013, -cy * res / 2 - 0.007)
    poses = window_poses(rng, res, cx, cy, origin, n)
    goals = [(float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8))) for _ in range(n)]
    p = plan.plan_params(robot_radius=min(0.3, res * 3))
    rec, cmds = check_plan(p, res, fields, origin, poses, goals, "default")
    if cx > 1:
        assert (rec["t_end"] == 0).any() and (rec["t_end"] == p.steps).any() and (rec["t_hit"] < p.steps).any()
        assert {c[3] for c in cmds} == {pd.OK, pd.BLOCKED}
    # extreme candidate sets: the smallest, and the largest on a few poses (the checker is plain Python)
    check_plan(plan.plan_params(n_v=1, n_w=1, steps=1, robot_radius=0.0), res, fields, origin, poses, goals, "1 x 1 x 1")
    big = plan.plan_params(n_v=16, n_w=65, steps=128, horizon=6.0, robot_radius=res * 2.5)
    check_plan(big, res, fields[:3], origin, [poses[0], poses[4], poses[1]], goals[:3], "16 x 65 x 128")


def test_invalid_calls_on_a_live_handle(jn):
    from jackal_navigation_amd import plan, _lib
    from jackal_navigation_amd.device import DeviceArray
    p = plan.plan_params()
    dF = DeviceArray.from_numpy(np.full((2, 32, 32), pd.FAR, np.uint16))
    L = plan._bind()
    INV = _lib.JN_ERR_INVALID
    with plan.Plan(p, 0.05, 32, 32, max_batch=2) as pl:
        org = (C.c_double * 2)(-0.8, -0.8)
        ok = (plan.Pose2D * 3)(plan.Pose2D(0, 0, 0), plan.Pose2D(0, 0, 0), plan.Pose2D(0, 0, 0))
        rec = np.full((3 * pl.K * 4,), 77, np.int32)
        goals = np.zeros((3, 2)); cmds = (plan.PlanCmd * 3)()
        for n, d, o, ps in ((0, dF.ptr, C.byref(org), ok), (3, dF.ptr, C.byref(org), ok), (-1, dF.ptr, C.byref(org), ok), (1, None, C.byref(org), ok),
                            (1, dF.ptr, None, ok), (1, dF.ptr, C.byref(org), None)):
            assert L.jn_plan_evaluate(pl._h, n, d, o, ps, rec.ctypes.data) == INV
            assert L.jn_plan_command(pl._h, n, d, o, ps, goals.ctypes.data, cmds, None) == INV
        assert L.jn_plan_evaluate(pl._h, 1, dF.ptr, C.byref(org), ok, None) == INV
        assert L.jn_plan_command(pl._h, 1, dF.ptr, C.byref(org), ok, None, cmds, None) == INV
        assert L.jn_plan_command(pl._h, 1, dF.ptr, C.byref(org), ok, goals.ctypes.data, None, None) == INV
        for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("nan")), (0.05 * 2.0 ** 30 * 1.01, 0, 0)):
            with pytest.raises(_lib.JnError) as e:
                pl.evaluate(dF.ptr, (-0.8, -0.8), [(0, 0, 0), bad])
            assert e.value.status == INV
        for bad_org in ((float("nan"), 0.0), (0.0, float("inf"))):
            with pytest.raises(_lib.JnError) as e:
                pl.evaluate(dF.ptr, bad_org, [(0, 0, 0)])
            assert e.value.status == INV
        with pytest.raises(_lib.JnError) as e:
            pl.command(dF.ptr, (-0.8, -0.8), [(0, 0, 0)], [(float("nan"), 0.0)])
        assert e.value.status == INV
        assert (rec == 77).all()                                                        # nothing was written by a refused call
        good = pl.evaluate(dF.ptr, (-0.8, -0.8), [(0, 0, 0), (0.1, 0.1, 1.0)])
        assert good.shape == (2, pl.K) and (good["t_hit"] == p.steps).all()


# ---- behaviour ----

def test_empty_map_goal_ahead_takes_the_fastest_straight_candidate(jn):
    from jackal_navigation_amd import plan
    p = plan.plan_params()
    grid = np.zeros((1, 256, 256), np.int8)
    field = gpu_clearance(grid, 20, 0)
    assert (field == pd.FAR).all()
    for theta in (0.0, 0.7, -2.0, math.pi):
        goal = (10.0 * math.cos(theta), 10.0 * math.sin(theta))
        rec, cmds = check_plan(p, 0.05, field, (-6.4, -6.4), [(0.0, 0.0, theta)], [goal])
        assert (rec["t_hit"] == p.steps).all() and (rec["t_end"] == p.steps).all() and (rec["min_d2"] == pd.FAR).all()
        assert cmds[0] == (p.v_max, 0.0, (p.n_v - 1) * p.n_w + (p.n_w - 1) // 2, pd.OK)


def test_a_wall_across_the_path_stops_the_straight_candidates_where_it_must(jn):
    """0.05 m cells, the grid's corner at (-1.025, -6.425) so that the straight arcs' points fall mid-cell; the wall fills column 40:
    x in [0.975, 1.025), for |y| <= 0.5 m only, so that turning arcs get round it.  robot_radius 0.31 -> r2 = floor(6.2^2) = 38 (0.3 / 0.05
    is 5.999999999999999 in double and would give 35): a hit is a point within 6 cells of the wall, column >= 34, x >= 0.675.  horizon 5 s: the straight candidates advance 0.05, 0.1 and 0.15 m per step and all
    three reach it: at steps 13 (0.70 m), 6 (0.70 m) and 4 (0.75 m)."""
    from jackal_navigation_amd import plan
    p = plan.plan_params(horizon=5.0, robot_radius=0.31)
    res, origin = 0.05, (-1.025, -6.425)
    grid = np.zeros((1, 256, 256), np.int8)
    grid[0, 118:140, 40] = 100
    field = gpu_clearance(grid, 20, 0)
    assert pd.r2_of(p, res) == 38 and pd.r2_of(plan.plan_params(), res) == 35
    rec, cmds = check_plan(p, res, field, origin, [(0.0, 0.0, 0.0)], [(6.0, 0.0)])
    m = (p.n_w - 1) // 2
    for iv in range(p.n_v):
        v = p.v_max * (iv + 1) / p.n_v
        xs = [v * (p.horizon * (s + 1) / p.steps) for s in range(p.steps)]
        want = next(s for s, x in enumerate(xs) if x >= 0.675)
        assert int(rec[0][iv * p.n_w + m]["t_hit"]) == want, (iv, want)
        assert int(rec[0][iv * p.n_w + m]["t_end"]) == p.steps
    assert [int(rec[0][iv * p.n_w + m]["t_hit"]) for iv in range(p.n_v)] == [13, 6, 4]
    v, w, k, status = cmds[0]
    assert status == pd.OK and w != 0.0 and int(rec[0][k]["t_hit"]) == p.steps and int(rec[0][k]["t_end"]) >= 1


def test_a_closed_box_around_the_robot_blocks_it(jn):
    from jackal_navigation_amd import plan
    p = plan.plan_params()
    grid = np.zeros((1, 128, 128), np.int8)
    grid[0, 54, 54:75] = grid[0, 74, 54:75] = grid[0, 54:75, 54] = grid[0, 54:75, 74] = 100     # a 1 m box, the robot in its middle
    field = gpu_clearance(grid, 20, 0)
    for theta in (0.0, 1.0, 2.5, -1.3):
        rec, cmds = check_plan(p, 0.05, field, (-3.225, -3.225), [(0.0, 0.0, theta)], [(3.0, 0.0)])
        assert (rec["t_hit"] < p.steps).all()
        assert cmds[0] == (0.0, 0.0, -1, pd.BLOCKED)
    # the same box of unknown cells blocks only when unknown counts as an obstacle
    grid[grid == 100] = -1
    _, cmds = check_plan(p, 0.05, gpu_clearance(grid, 20, 1), (-3.225, -3.225), [(0.0, 0.0, 0.0)], [(3.0, 0.0)])
    assert cmds[0][3] == pd.BLOCKED
    _, cmds = check_plan(p, 0.05, gpu_clearance(grid, 20, 0), (-3.225, -3.225), [(0.0, 0.0, 0.0)], [(3.0, 0.0)])
    assert cmds[0] == (p.v_max, 0.0, (p.n_v - 1) * p.n_w + (p.n_w - 1) // 2, pd.OK)


# ---- end to end ----

def test_end_to_end_behind_the_local_map(jn):
    """The driving scene of test_gpu_localmap.py on exact disparities: updates over several poses, then the clearance of the map's grid on
    the device (no host round trip) and the plan — equal to the checker run on the checker's own map."""
    from jackal_navigation_amd import localmap, node, plan
    from test_gpu_localmap import drive_scene
    W, H = 320, 180
    sp = node.scan_params(W, H)
    floor, wall = drive_scene(sp, W, H)
    lp = localmap.localmap_params(ld.I16_SUB)
    ref = ld.Map(lp)
    poses = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.02), (0.1, 0.01, 0.05), (0.1, 0.01, 0.8), (0.1, 0.01, -0.8)]
    maps = np.stack([wall, wall, wall, floor, floor])
    p = plan.plan_params(horizon=4.0)
    with localmap.LocalMap(lp, max_batch=5) as m, plan.Plan(p, lp.resolution, lp.cells_x, lp.cells_y) as pl:
        from jackal_navigation_amd.device import DeviceArray
        dD = DeviceArray.from_numpy(maps)
        m.update(sp, poses, dD.ptr, W, H)
        ref.update(sp, poses, maps)
        assert np.array_equal(m.read()[1], ref.grid()) and (ref.grid() == 100).sum() >= 10
        for R, unk in ((20, 0), (8, 1), (64, 0)):
            dF = plan.localmap_clearance(m, R, unk)
            want_field = pd.clearance(ref.grid(), R, unk)
            assert np.array_equal(dF.numpy(), want_field), (R, unk)
            origin = m.window().origin
            assert origin == (float(ref.g0[0]) * lp.resolution, float(ref.g0[1]) * lp.resolution)
            for pose, goal in (((0.1, 0.01, 0.05), (4.0, 0.0)), ((0.1, 0.01, 0.8), (4.0, 0.0)), ((1.0, -0.5, 3.0), (-3.0, 1.0))):
                cmds, rec = pl.command(dF.ptr, origin, [pose], [goal], with_records=True)
                want = pd.rollout(p, lp.resolution, want_field, origin, pose)
                assert np.array_equal(rec[0], want), (R, unk, pose)
                c = cmds[0]
                assert (c.v, c.w, c.candidate, c.status) == pd.choose(p, lp.resolution, want, pose, goal), (R, unk, pose)
            if (R, unk) == (20, 0):
                # facing the remembered wall 2 m ahead: the fastest straight candidate is stopped by it, and the planner turns or slows
                mid = (p.n_v - 1) * p.n_w + (p.n_w - 1) // 2
                cmds, rec = pl.command(dF.ptr, origin, [(0.1, 0.01, 0.0)], [(4.0, 0.0)], with_records=True)
                assert rec[0][mid]["t_hit"] < p.steps and cmds[0].candidate != mid
                tw = plan.twist_message(cmds[0])
                assert tw["linear"]["x"] == cmds[0].v and tw["angular"]["z"] == cmds[0].w
            dF.free()
            # the caller's own output buffer
            mine = DeviceArray.from_numpy(np.full((lp.cells_y, lp.cells_x), POISON, np.uint16))
            assert plan.localmap_clearance(m, R, unk, mine.ptr) is None and np.array_equal(mine.numpy(), want_field)


def test_end_to_end_behind_the_subpixel_costmap(jn):
    """A jn_subpix_costmap batch in the robot frame: its device grids -> clearance -> plan under the zero pose with the costmap's origin.
    The checker's grid is 100 where subpix_def's hits reach min_hits; the free / unknown split of the other cells hangs on an atan2 and
    does not matter here (unknown_is_obstacle = 0)."""
    from jackal_navigation_amd import costmap, node, plan, subpix
    from jackal_navigation_amd.device import DeviceArray
    from test_gpu_localmap import drive_scene
    W, H, n = 320, 180, 3
    sp = node.scan_params(W, H)
    floor, wall = drive_scene(sp, W, H)
    near = floor.copy()
    near[40:120, 100:140] = sd.wall_q(sp, W, H, 1.2)[0][40:120, 100:140]
    maps = np.stack([wall, floor, near])
    cp = costmap.costmap_params()
    fp = subpix.subpix_params(sd.I16_SUB)
    dD = DeviceArray.from_numpy(maps)
    bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    hits = DeviceArray((n, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((n, cp.cells_y, cp.cells_x), np.int8)
    subpix.subpix_costmap(sp, cp, fp, n, dD.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr)
    dF = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), POISON, np.uint16))
    plan.clearance(grid.ptr, 20, 0, n, cp.cells_x, cp.cells_y, dF.ptr)
    want_grid = np.stack([np.where(sd.hits(sp, cp, *sd.to_q(maps[f], sd.I16_SUB)) >= cp.min_hits, 100, -1).astype(np.int8) for f in range(n)])
    assert np.array_equal(grid.numpy() == 100, want_grid == 100) and (want_grid[0] == 100).any() and (want_grid[2] == 100).any()
    want_field = pd.clearance_batch(want_grid, 20, 0)
    assert np.array_equal(dF.numpy(), want_field)
    p = plan.plan_params(horizon=4.0)
    origin = (cp.origin_x, cp.origin_y)
    zero = [(0.0, 0.0, 0.0)] * n
    goals = [(5.0, 0.0), (5.0, 0.0), (5.0, 1.0)]
    with plan.Plan(p, cp.resolution, cp.cells_x, cp.cells_y, max_batch=n) as pl:
        cmds, rec = pl.command(dF.ptr, origin, zero, goals, with_records=True)
    mid = (p.n_v - 1) * p.n_w + (p.n_w - 1) // 2
    for f in range(n):
        want = pd.rollout(p, cp.resolution, want_field[f], origin, zero[f])
        assert np.array_equal(rec[f], want), f
        c = cmds[f]
        assert (c.v, c.w, c.candidate, c.status) == pd.choose(p, cp.resolution, want, zero[f], goals[f]), f
    assert rec[0][mid]["t_hit"] < p.steps and rec[1][mid]["t_hit"] == p.steps and cmds[1].candidate == mid

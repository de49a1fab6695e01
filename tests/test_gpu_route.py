"""The cost-to-go field (include/jn_route.h) on the GPU against its definition (tests/route_def.py: Dijkstra with a heap), everything bit for
bit and every output poisoned beforehand: the field and the seed counts, the gathered togo values, the chosen commands, the dead-end
scenario of tests/test_route_api.py command for command; end to end behind the local map and behind the sub-pixel costmap.

Kernel forms (csrc/route.hip), each asserted through jn_route_stats.form where it is expected:
  whole   k_route_relax<true>, one launch, one workgroup per frame with the grid in LDS: every grid here up to 256 x 256, and the thin
          ones (1 x 512, 512 x 1).  Inside it the sizes cover rows and columns shorter than a wave and than the workgroup (1, 37, 53),
          bit-plane words that end inside a row (37, 53), one thread per row / column up to 512.
  tiled   k_route_init, launches of k_route_relax<false> in batches, k_route_final: 512 x 512 (four tiles of 256 x 256) and 300 x 280
          (four tiles of 150 x 140: ragged tiles, borders exchanged through global memory).  The serpentines and the spiral make a path
          cross tile borders hundreds of times, so the batches run long; the open grids end inside the first batch."""
import ctypes as C
import math

import numpy as np
import pytest

import localmap_def as ld
import plan_def as pd
import route_def as rd
import subpix_def as sd
from test_gpu_plan import gpu_clearance, random_grids, window_poses
from test_route_api import DEAD_END_CYCLES, DEAD_END_DT, DEAD_END_RADIUS, DEAD_END_TOLERANCE, dead_end_scene

pytestmark = pytest.mark.gpu

POISON = 0xABCD


def params(**kw):
    """-> (jn_route_params, the definition's Params) with the same fields."""
    from jackal_navigation_amd import route
    return route.route_params(**kw), rd.Params(**kw)


def gpu_field(d2s, r2, rp, goals):
    """n fields through the device-pointer form of route.costtogo, the output poisoned beforehand -> (g, seeds, stats)."""
    from jackal_navigation_amd import route
    from jackal_navigation_amd.device import DeviceArray
    n, cy, cx = d2s.shape
    dD = DeviceArray.from_numpy(np.ascontiguousarray(d2s, np.uint16))
    dG = DeviceArray.from_numpy(np.full((n, cy, cx), POISON, np.uint16))
    seeds, st = route.costtogo(dD.ptr, r2, rp, goals, n, cx, cy, dG.ptr, with_stats=True)
    out = dG.numpy()
    dD.free(); dG.free()
    return out, seeds, st


def check_field(d2s, r2, kw, goals, what, form=None):
    from jackal_navigation_amd import route
    rp, dp = params(**kw)
    got, seeds, st = gpu_field(d2s, r2, rp, goals)
    assert got.dtype == np.uint16 and got.shape == d2s.shape
    if form is not None:
        assert st.form == form, (what, st.form)
    assert st.launches >= 1 and st.rounds >= 1
    for f in range(d2s.shape[0]):
        want, ws = rd.field(d2s[f], r2, dp, goals[f])
        assert int(seeds[f]) == ws, (what, r2, kw, f, int(seeds[f]), ws)
        assert np.array_equal(got[f], want), (what, r2, kw, f, goals[f], int((got[f] != want).sum()))
        assert (ws == 0) == bool((want == rd.UNREACHED).all())
    return got, st


def expected_form(cy, cx):
    from jackal_navigation_amd import route
    return route.FORM_WHOLE if cy * cx <= 256 * 256 or min(cy, cx) == 1 else route.FORM_TILED


FIELD_CASES = [
    # cy, cx, n, densities, [(r2, near_radius, near_penalty, goal_radius)]
    (1, 1, 3, (0, 1.0), [(0, 10, 3, 2), (36, 0, 0, 0)]),
    (1, 512, 3, (0, 0.002, 0.01), [(0, 10, 3, 2), (36, 3, 64, 0), (0, 255, 64, 16)]),
    (512, 1, 3, (0, 0.002, 0.01), [(0, 10, 3, 2), (36, 3, 64, 0), (65025, 0, 0, 16)]),
    (53, 37, 32, (0, 0.001, 0.01, 0.1, 0.5, 0.95), [(r2, 4, pen, gr) for r2 in (0, 36, 65025) for pen in (0, 3, 64) for gr in (0, 2, 16)]),
    (37, 53, 1, (0.02,), [(0, 10, 3, 2), (36, 10, 64, 16)]),
    (128, 128, 32, (0, 0.0005, 0.005, 0.05, 0.5), [(36, 10, 3, 2), (0, 2, 64, 0)]),
    (256, 256, 3, (0, 0.001, 0.3), [(36, 10, 3, 2), (0, 1, 64, 16), (65025, 10, 0, 0)]),
    (300, 280, 2, (0.002, 0.2), [(36, 10, 3, 2), (0, 1, 64, 0)]),
    (512, 512, 2, (0.0006, 0.3), [(36, 10, 3, 2), (0, 1, 64, 16), (65025, 0, 0, 0)]),
]


@pytest.mark.parametrize("cy,cx,n,dens,combos", FIELD_CASES, ids=["%dx%dx%d" % (c[2], c[0], c[1]) for c in FIELD_CASES])
def test_field_equals_the_definition_on_random_grids(jn, cy, cx, n, dens, combos):
    """The density mix of test_gpu_plan.random_grids; the clearance fields are the device's own (checked there), radius 255 so that
    r2 = 65025 means something.  A different goal per frame."""
    rng = np.random.default_rng(31 * cy + cx + n)
    grids = random_grids(rng, n, cy, cx, dens)
    d2s = gpu_clearance(grids, 255, 0)
    goals = [(int(rng.integers(0, cx)), int(rng.integers(0, cy))) for _ in range(n)]
    assert n == 1 or cx * cy == 1 or len(set(goals)) > 1
    for r2, nr, pen, gr in combos:
        check_field(d2s, r2, dict(near_radius=nr, near_penalty=pen, goal_radius=gr), goals, (cy, cx, n), expected_form(cy, cx))


# ---- structured worst cases ----

def serpentine(cy, cx):
    """Corridors one cell wide on the even rows, walls on the odd ones with one gap each, at alternating ends: one path through every cell."""
    g = np.zeros((cy, cx), np.int8)
    g[1::2, :] = 100
    for k, row in enumerate(range(1, cy, 2)):
        g[row, cx - 1 if k % 2 == 0 else 0] = 0
    return g


def spiral(cy, cx):
    """A corridor one cell wide wound inward from (0, 0), carved by a turtle that turns right when the cell ahead, or the one behind it,
    is already corridor."""
    g = np.full((cy, cx), 100, np.int8)
    x, y, dx, dy = 0, 0, 1, 0
    g[0, 0] = 0

    def can(dx, dy):
        nx, ny = x + dx, y + dy
        if not (0 <= nx < cx and 0 <= ny < cy) or g[ny, nx] == 0:
            return False
        ax, ay = nx + dx, ny + dy
        return not (0 <= ax < cx and 0 <= ay < cy and g[ay, ax] == 0)

    while True:
        if not can(dx, dy):
            dx, dy = -dy, dx
            if not can(dx, dy):
                return g, (x, y)
        x, y = x + dx, y + dy
        g[y, x] = 0


def comb(cy, cx):
    """A corridor along row 0 with a dead-end tooth down every even column."""
    g = np.zeros((cy, cx), np.int8)
    g[2:, 1::2] = 100
    g[1, 1::2] = 100
    return g


@pytest.mark.parametrize("side", [256, 512])
def test_structured_worst_cases(jn, side):
    from jackal_navigation_amd import route
    form = expected_form(side, side)
    free = dict(near_radius=0, near_penalty=0, goal_radius=0)
    # the serpentine, the goal at its far end: the most rounds (whole form) and the most launches (tiled form)
    s = serpentine(side, side)
    d2 = gpu_clearance(s[None], 2, 0)
    got, st = check_field(d2, 0, free, [(0, 0)], ("serpentine", side), form)
    # (5 per cell: the cut at 65534 ends the field after 13 106 cells, 51 corridors of 256 cells or 25 of 512 — it bounds the rounds too)
    assert st.rounds > 20 and (got[0][s == 0] == rd.UNREACHED).any() and int(got[0][got[0] != rd.UNREACHED].max()) > 65534 - 7
    if form == route.FORM_TILED:
        assert st.launches > 20
    # the goal in the middle of the serpentine: both ways at once
    check_field(d2, 0, free, [(side // 2, side // 2)], ("serpentine mid", side), form)
    # the same serpentine with every corridor cell in the penalty band (d2 = 1 next to a wall): 69 per step, the far end above 65534
    band = dict(near_radius=1, near_penalty=64, goal_radius=0)
    want, _ = rd.field(d2[0], 0, rd.Params(**band), (0, 0))
    reached = want != rd.UNREACHED
    assert reached.sum() > 900 and (~reached & (s == 0)).sum() > 900            # the definition does cross the cut on this input
    assert 65534 - 71 < int(want[reached].max()) <= 65534            # a step costs 69, or 71 round a corner
    check_field(d2, 0, band, [(0, 0)], ("serpentine cut", side), form)
    # the spiral, from its centre and from its mouth
    sp, centre = spiral(side, side)
    d2 = gpu_clearance(sp[None], 2, 0)
    check_field(np.concatenate([d2, d2]), 0, free, [centre, (0, 0)], ("spiral", side), form)
    # the comb: every tooth a dead end
    d2 = gpu_clearance(comb(side, side)[None], 2, 0)
    check_field(np.concatenate([d2, d2]), 0, free, [(side - 2, side - 1), (0, 0)], ("comb", side), form)


def test_goals_on_borders_clamped_blocked_and_a_frame_without_a_passable_cell(jn):
    from jackal_navigation_amd import route
    rng = np.random.default_rng(77)
    for cy, cx in ((128, 96), (300, 280)):
        grids = random_grids(rng, 2, cy, cx, (0.003, 0.05))
        d2 = gpu_clearance(grids, 20, 0)
        res, org = 0.05, (-1.0, 2.0)
        # corners, border cells, and goals beyond the map clamped onto it by jn_route_goal_cell
        worlds = [(-50.0, -50.0), (50.0, 50.0), (-50.0, 50.0), (50.0, -50.0), (org[0] + 0.5 * cx * res, 1e9), (-1e9, org[1] + 0.3 * cy * res)]
        cells = [route.goal_cell(res, cx, cy, org, w) for w in worlds]
        assert cells[:4] == [(0, 0), (cx - 1, cy - 1), (0, cy - 1), (cx - 1, 0)] and cells[4][1] == cy - 1 and cells[5][0] == 0
        assert cells == [rd.goal_cell(res, cx, cy, org, w) for w in worlds]
        cells += [(cx // 2, 0), (cx - 1, cy // 2)]
        for gr in (0, 2, 16):
            for k in range(0, len(cells), 2):
                check_field(d2, 9, dict(goal_radius=gr), cells[k:k + 2], ("border", cy, cx, gr), expected_form(cy, cx))
        # blocked goals: on an obstacle cell, goal_radius 0 -> no seeds, the field all UNREACHED
        oy, ox = (int(v[0]) for v in np.nonzero(grids[1] == 100))
        got, seeds, _ = gpu_field(d2, 9, params(goal_radius=0)[0], [(ox, oy), (ox, oy)])
        assert int(seeds[1]) == 0 and (got[1] == rd.UNREACHED).all()
        check_field(d2, 9, dict(goal_radius=0), [(ox, oy), (ox, oy)], ("blocked", cy, cx))
        # a frame with no passable cell at all next to an ordinary one
        full = grids.copy(); full[0] = 100
        d2f = gpu_clearance(full, 20, 0)
        got, st = check_field(d2f, 0, dict(), [(3, 3), (3, 3)], ("full", cy, cx))
        assert (got[0] == rd.UNREACHED).all()
        # an empty grid: FAR everywhere, the chamfer distance
        d2e = np.full((1, cy, cx), pd.FAR, np.uint16)
        got, st = check_field(d2e, 65025, dict(goal_radius=0), [(5, 7)], ("empty", cy, cx))
        ys, xs = np.mgrid[0:cy, 0:cx]
        dx, dy = np.abs(xs - 5), np.abs(ys - 7)
        assert np.array_equal(got[0], 7 * np.minimum(dx, dy) + 5 * np.abs(dx - dy))


def test_repeatable_numpy_form_and_invalid_calls(jn):
    from jackal_navigation_amd import route, _lib
    from jackal_navigation_amd.device import DeviceArray
    rng = np.random.default_rng(3)
    d2 = gpu_clearance(random_grids(rng, 2, 200, 300, (0.01,)), 20, 0)
    rp = route.route_params()
    goals = [(10, 10), (250, 150)]
    a, sa, _ = gpu_field(d2, 36, rp, goals)
    b, sb, _ = gpu_field(d2, 36, rp, goals)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    g, s = route.costtogo(d2, 36, rp, goals)
    assert np.array_equal(g, a) and np.array_equal(s, sa)
    g1, s1 = route.costtogo(d2[1], 36, rp, goals[1])                    # a 2-D field gives a 2-D field
    assert g1.shape == (200, 300) and np.array_equal(g1, a[1]) and int(s1[0]) == int(sa[1])
    # an invalid call leaves the output alone
    dD = DeviceArray.from_numpy(d2); dG = DeviceArray.from_numpy(np.full(d2.shape, POISON, np.uint16))
    for bad in (dict(r2=-1), dict(r2=65026), dict(n=0), dict(cx=0), dict(cy=513), dict(goals=[(300, 0), (0, 0)]), dict(goals=[(0, 0), (0, 200)])):
        kw = dict(r2=36, n=2, cx=300, cy=200, goals=goals); kw.update(bad)
        with pytest.raises(_lib.JnError) as e:
            route.costtogo(dD.ptr, kw["r2"], rp, kw["goals"], kw["n"], kw["cx"], kw["cy"], dG.ptr)
        assert e.value.status == _lib.JN_ERR_INVALID
    assert (dG.numpy() == POISON).all()


# ---- evaluation and command ----

def check_route(p, res, d2s, gs, origin, poses, what):
    """jn_route_command, jn_route_evaluate and jn_plan_evaluate on device fields against the definitions."""
    from jackal_navigation_amd import plan, route
    from jackal_navigation_amd.device import DeviceArray
    n, cy, cx = d2s.shape
    dD, dG = DeviceArray.from_numpy(d2s), DeviceArray.from_numpy(gs)
    with plan.Plan(p, res, cx, cy, max_batch=n) as pl:
        rt = route.Route(pl)
        cmds, rec, togo = rt.command(dD.ptr, dG.ptr, origin, poses, with_records=True)
        rec2, togo2 = rt.evaluate(dD.ptr, dG.ptr, origin, poses)
        assert np.array_equal(rec, rec2) and np.array_equal(togo, togo2)
        assert np.array_equal(rec, pl.evaluate(dD.ptr, origin, poses))                    # jn_plan_evaluate's records, bit for bit
        assert [(c.v, c.w, c.candidate, c.status) for c in rt.command(dD.ptr, dG.ptr, origin, poses)] == [(c.v, c.w, c.candidate, c.status) for c in cmds]
    dD.free(); dG.free()
    out = []
    for f in range(n):
        want = pd.rollout(p, res, d2s[f], origin, poses[f])
        assert np.array_equal(rec[f], want), (what, f)
        wt = rd.gather(gs[f], want)
        assert togo.dtype == np.uint16 and np.array_equal(togo[f], wt), (what, f)
        wc = rd.choose(p, res, want, wt)
        c = cmds[f]
        assert (c.candidate, c.status) == wc[2:], (what, f, wc)
        assert np.array_equal(np.array([c.v, c.w]).view(np.uint64), np.array(wc[:2]).view(np.uint64)), (what, f)
        assert np.array_equal(np.array([route.choose(p, res, rec[f], togo[f]).v]).view(np.uint64), np.array(wc[:1]).view(np.uint64))
        out.append(wc)
    return rec, togo, out


@pytest.mark.parametrize("cy,cx,res,R,dens", [(256, 256, 0.05, 20, 0.01), (53, 37, 0.1, 64, 0.01), (1, 1, 2.0, 3, 0), (512, 512, 0.03, 20, 0.005)])
def test_records_togo_and_commands_equal_the_definition(jn, cy, cx, res, R, dens):
    from jackal_navigation_amd import plan
    rng = np.random.default_rng(9 * cy + cx)
    n = 16
    grids = random_grids(rng, 2, cy, cx, (dens,))
    p = plan.plan_params(robot_radius=min(0.3, res * 3))
    r2 = pd.r2_of(p, res)
    d2s = gpu_clearance(grids, R, 0)[np.arange(n) % 2]
    origin = (-cx * res / 2 + 0.013, -cy * res / 2 - 0.007)
    goals = [(int(rng.integers(0, cx)), int(rng.integers(0, cy))) for _ in range(n)]
    gs, _, _ = gpu_field(d2s, r2, params()[0], goals)                                     # the device's own fields, checked above
    poses = window_poses(rng, res, cx, cy, origin, n)
    rec, togo, cmds = check_route(p, res, d2s, gs, origin, poses, "default")
    if cx > 1:
        assert (togo == rd.UNREACHED).any() and (togo != rd.UNREACHED).any() and {c[3] for c in cmds} == {pd.OK, pd.BLOCKED}
    check_route(plan.plan_params(n_v=1, n_w=1, steps=1, robot_radius=0.0), res, d2s, gs, origin, poses, "1 x 1 x 1")
    check_route(plan.plan_params(n_v=16, n_w=65, steps=128, horizon=6.0, robot_radius=res * 2.5), res, d2s[:2], gs[:2], origin, [poses[0], poses[4]],
                "16 x 65 x 128")


def test_invalid_calls_on_a_live_handle(jn):
    from jackal_navigation_amd import plan, route, _lib
    from jackal_navigation_amd.device import DeviceArray
    p = plan.plan_params()
    dF = DeviceArray.from_numpy(np.full((2, 32, 32), pd.FAR, np.uint16))
    dG = DeviceArray.from_numpy(np.zeros((2, 32, 32), np.uint16))
    L = route._bind()
    INV = _lib.JN_ERR_INVALID
    with plan.Plan(p, 0.05, 32, 32, max_batch=2) as pl:
        rt = route.Route(pl)
        org = (C.c_double * 2)(-0.8, -0.8)
        ok = (plan.Pose2D * 3)(plan.Pose2D(0, 0, 0), plan.Pose2D(0, 0, 0), plan.Pose2D(0, 0, 0))
        rec = np.full((3 * pl.K * 4,), 77, np.int32); togo = np.full(3 * pl.K, 77, np.uint16)
        cmds = (plan.PlanCmd * 3)()
        for n, d, g, o, ps in ((0, dF.ptr, dG.ptr, C.byref(org), ok), (3, dF.ptr, dG.ptr, C.byref(org), ok), (1, None, dG.ptr, C.byref(org), ok),
                               (1, dF.ptr, None, C.byref(org), ok), (1, dF.ptr, dG.ptr, None, ok), (1, dF.ptr, dG.ptr, C.byref(org), None)):
            assert L.jn_route_evaluate(pl._h, n, d, g, o, ps, rec.ctypes.data, togo.ctypes.data) == INV
            assert L.jn_route_command(pl._h, n, d, g, o, ps, cmds, None, None) == INV
        assert L.jn_route_evaluate(pl._h, 1, dF.ptr, dG.ptr, C.byref(org), ok, None, togo.ctypes.data) == INV
        assert L.jn_route_evaluate(pl._h, 1, dF.ptr, dG.ptr, C.byref(org), ok, rec.ctypes.data, None) == INV
        assert L.jn_route_command(pl._h, 1, dF.ptr, dG.ptr, C.byref(org), ok, None, None, None) == INV
        for bad in ((float("nan"), 0, 0), (0, 0, float("inf"))):
            with pytest.raises(_lib.JnError) as e:
                rt.evaluate(dF.ptr, dG.ptr, (-0.8, -0.8), [(0, 0, 0), bad])
            assert e.value.status == INV
        assert (rec == 77).all() and (togo == 77).all()                                  # nothing was written by a refused call
        r, t = rt.evaluate(dF.ptr, dG.ptr, (-0.8, -0.8), [(0, 0, 0), (0.1, 0.1, 1.0)])
        assert r.shape == (2, pl.K) and t.shape == (2, pl.K) and (t[r["last_cell"] >= 0] == 0).all() and (t[r["last_cell"] < 0] == rd.UNREACHED).all()


# ---- end to end ----

def test_end_to_end_behind_the_local_map(jn):
    """The driving scene of test_gpu_localmap.py: updates over several poses, then clearance and cost-to-go of the map's grid on the device
    (localmap_costtogo: no host round trip) and the command — equal to the definitions run on the checker's own map."""
    from jackal_navigation_amd import localmap, node, plan, route
    from jackal_navigation_amd.device import DeviceArray
    from test_gpu_localmap import drive_scene
    W, H = 320, 180
    sp = node.scan_params(W, H)
    floor, wall = drive_scene(sp, W, H)
    lp = localmap.localmap_params(ld.I16_SUB)
    ref = ld.Map(lp)
    poses = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.02), (0.1, 0.01, 0.05), (0.1, 0.01, 0.8), (0.1, 0.01, -0.8)]
    maps = np.stack([wall, wall, wall, floor, floor])
    p = plan.plan_params(horizon=4.0)
    r2 = pd.r2_of(p, lp.resolution)
    with localmap.LocalMap(lp, max_batch=5) as m, plan.Plan(p, lp.resolution, lp.cells_x, lp.cells_y) as pl:
        dD = DeviceArray.from_numpy(maps)
        m.update(sp, poses, dD.ptr, W, H)
        ref.update(sp, poses, maps)
        assert np.array_equal(m.read()[1], ref.grid()) and (ref.grid() == 100).sum() >= 10
        origin = m.window().origin
        rt = route.Route(pl)
        for kw, unk, goal in ((dict(), 0, (4.0, 0.0)), (dict(near_radius=4, near_penalty=64, goal_radius=0), 1, (3.0, 1.0)), (dict(goal_radius=16), 0, (40.0, -40.0))):
            rp, dp = params(**kw)
            dD2, dTogo, seeds, cell = route.localmap_costtogo(m, p, goal, rp, unknown_is_obstacle=unk)
            radius = route.min_clearance_radius(r2, rp)
            want_d2 = pd.clearance(ref.grid(), radius, unk)
            assert cell == rd.goal_cell(lp.resolution, lp.cells_x, lp.cells_y, origin, goal)
            want_g, want_seeds = rd.field(want_d2, r2, dp, cell)
            assert np.array_equal(dD2.numpy(), want_d2) and seeds == want_seeds and np.array_equal(dTogo.numpy(), want_g), kw
            for pose in ((0.1, 0.01, 0.05), (0.1, 0.01, 0.8), (1.0, -0.5, 3.0)):
                cmds, rec, togo = rt.command(dD2.ptr, dTogo.ptr, origin, [pose], with_records=True)
                want = pd.rollout(p, lp.resolution, want_d2, origin, pose)
                wt = rd.gather(want_g, want)
                assert np.array_equal(rec[0], want) and np.array_equal(togo[0], wt), (kw, pose)
                c = cmds[0]
                assert (c.v, c.w, c.candidate, c.status) == rd.choose(p, lp.resolution, want, wt), (kw, pose)
            dD2.free(); dTogo.free()
        with pytest.raises(ValueError):
            route.localmap_costtogo(m, p, (4.0, 0.0), radius=5)                           # below what r2 and near_radius need


def test_end_to_end_behind_the_subpixel_costmap(jn):
    """A jn_subpix_costmap batch in the robot frame: its device grids -> clearance -> cost-to-go -> command under the zero pose with the
    costmap's origin, all on device pointers.  (unknown_is_obstacle = 0, as in test_gpu_plan.py.)"""
    from jackal_navigation_amd import costmap, node, plan, route, subpix
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
    dG = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), POISON, np.uint16))
    plan.clearance(grid.ptr, 20, 0, n, cp.cells_x, cp.cells_y, dF.ptr)
    p = plan.plan_params(horizon=4.0)
    r2 = pd.r2_of(p, cp.resolution)
    rp, dp = params()
    origin = (cp.origin_x, cp.origin_y)
    goals = [(5.0, 0.0), (5.0, 0.0), (5.0, 1.0)]
    cells = [route.goal_cell(cp.resolution, cp.cells_x, cp.cells_y, origin, g) for g in goals]
    seeds = route.costtogo(dF.ptr, r2, rp, cells, n, cp.cells_x, cp.cells_y, dG.ptr)
    want_grid = np.stack([np.where(sd.hits(sp, cp, *sd.to_q(maps[f], sd.I16_SUB)) >= cp.min_hits, 100, -1).astype(np.int8) for f in range(n)])
    want_d2 = pd.clearance_batch(want_grid, 20, 0)
    assert np.array_equal(dF.numpy(), want_d2)
    want_g, want_seeds = rd.field_batch(want_d2, r2, dp, cells)
    assert np.array_equal(dG.numpy(), want_g) and seeds.tolist() == want_seeds
    zero = [(0.0, 0.0, 0.0)] * n
    with plan.Plan(p, cp.resolution, cp.cells_x, cp.cells_y, max_batch=n) as pl:
        cmds, rec, togo = route.Route(pl).command(dF.ptr, dG.ptr, origin, zero, with_records=True)
    for f in range(n):
        want = pd.rollout(p, cp.resolution, want_d2[f], origin, zero[f])
        wt = rd.gather(want_g[f], want)
        assert np.array_equal(rec[f], want) and np.array_equal(togo[f], wt), f
        c = cmds[f]
        assert (c.v, c.w, c.candidate, c.status) == rd.choose(p, cp.resolution, want, wt), f


def test_the_dead_end_through_the_library(jn):
    """tests/test_route_api.py's scenario with every step made by the library: jn_clearance and jn_route_field once on the static map,
    jn_route_command per cycle.  The trajectory equals the definition's, command for command, and arrives; jn_plan_command on the same
    field does not."""
    from jackal_navigation_amd import plan, route
    from jackal_navigation_amd.device import DeviceArray
    grid, res, origin, start, goal = dead_end_scene()
    p = plan.plan_params()
    rp, dp = params()
    r2 = pd.r2_of(p, res)
    d2 = gpu_clearance(grid[None], DEAD_END_RADIUS, 0)
    want_d2 = pd.clearance(grid, DEAD_END_RADIUS)
    assert np.array_equal(d2[0], want_d2)
    cell = route.goal_cell(res, 256, 256, origin, goal)
    g, seeds, st = gpu_field(d2, r2, rp, [cell])
    want_g, want_seeds = rd.field(want_d2, r2, dp, cell)
    assert np.array_equal(g[0], want_g) and int(seeds[0]) == want_seeds == 13 and st.form == route.FORM_WHOLE
    dD, dG = DeviceArray.from_numpy(d2), DeviceArray.from_numpy(g)

    def run(command, want_command):
        pose, n = start, 0
        for n in range(DEAD_END_CYCLES):
            if math.hypot(pose[0] - goal[0], pose[1] - goal[1]) <= DEAD_END_TOLERANCE:
                return "arrived", n, pose
            c = command(pose)
            want = want_command(pose)
            assert (c.v, c.w, c.candidate, c.status) == want, (n, pose, want)
            if c.status != pd.OK:
                return "blocked", n, pose
            pose = rd.advance(pose, c.v, c.w, DEAD_END_DT)
            assert int(want_d2.reshape(-1)[pd.cell_of(pose[0], pose[1], origin, res, 256, 256)]) > r2
        return "timeout", n + 1, pose

    def want_route(pose):
        rec = pd.rollout(p, res, want_d2, origin, pose)
        return rd.choose(p, res, rec, rd.gather(want_g, rec))

    with plan.Plan(p, res, 256, 256) as pl:
        rt = route.Route(pl)
        outcome, n, pose = run(lambda q: rt.command(dD.ptr, dG.ptr, origin, [q])[0], want_route)
        assert outcome == "arrived" and n < 60, (outcome, n, pose)
        outcome, n, pose = run(lambda q: pl.command(dD.ptr, origin, [q], [goal])[0],
                               lambda q: pd.choose(p, res, pd.rollout(p, res, want_d2, origin, q), q, goal))
        assert outcome in ("blocked", "timeout") and math.hypot(pose[0] - goal[0], pose[1] - goal[1]) > DEAD_END_TOLERANCE
    # the path the library traces from the start is the definition's
    sc = route.goal_cell(res, 256, 256, origin, start[:2])
    cells, status = route.trace(g[0], d2[0], r2, rp, sc)
    assert status == route.OK and cells.tolist() == rd.trace(want_g, want_d2, r2, dp, sc)[0]
    msg = route.path_message(cells, origin, res, 256)
    assert len(msg["poses"]) == len(cells) and abs(msg["poses"][-1]["pose"]["position"]["x"] - goal[0]) <= 3 * res

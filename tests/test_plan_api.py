"""The local planner's C ABI (include/jn_plan.h), its Python mirror and its numpy definition (tests/plan_def.py): exports, struct layout,
defaults, argument checking, the templates and the chooser (both are host code: compared bit for bit here), and the definition on cases
small enough to do by hand.  No GPU needed; the kernels are compared in tests/test_gpu_plan.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import plan_def as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jn_plan.h")


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_by_both_libraries(jn):
    from jackal_navigation_amd import plan
    declared = _declared_functions()
    assert declared == sorted(plan.PLAN_EXPORTS) == sorted(jn.PLAN_EXPORTS)
    assert len(declared) == 8
    lib = jn.load()
    assert not [n for n in declared if not hasattr(lib, n)]
    with jn.hooks_library() as hooks:
        assert hooks is not lib
        assert not [n for n in declared if not hasattr(hooks, n)]
    for name in ("Plan", "PlanParams", "PlanRecord", "PlanCmd", "plan_params"):
        assert hasattr(jn, name), name
    for name in ("evaluate", "command", "close"):
        assert hasattr(jn.Plan, name), name
    for name in ("clearance", "localmap_clearance", "templates", "choose", "twist_message"):
        assert hasattr(plan, name), name
    assert jn.load().jn_version() == b"jn_stereo 0.4 (gfx950)"
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "jn.PLAN_EXPORTS" in entry                                  # build() checks these symbols too


def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [f.strip() for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for f in decl.split(",")]


def test_struct_layout_defaults_and_constants(jn):
    from jackal_navigation_amd import plan, costmap
    text = open(HEADER).read()
    P, R, Cm = plan.PlanParams, plan.PlanRecord, plan.PlanCmd
    assert (C.sizeof(P), C.sizeof(R), C.sizeof(Cm)) == (80, 16, 24)
    want = ["v_max", "w_max", "horizon", "robot_radius", "w_goal", "w_clear", "w_speed", "clear_cap", "n_v", "n_w", "steps", "reserved"]
    assert [n for n, _ in P._fields_] == want == _struct_fields(text, "jn_plan_params")
    assert [getattr(P, n).offset for n in want] == list(range(0, 64, 8)) + [64, 68, 72, 76]
    assert [n for n, _ in R._fields_] == ["t_end", "t_hit", "min_d2", "last_cell"] == _struct_fields(text, "jn_plan_record")
    assert [getattr(R, n).offset for n, _ in R._fields_] == [0, 4, 8, 12]
    assert [n for n, _ in Cm._fields_] == ["v", "w", "candidate", "status"] == _struct_fields(text, "jn_plan_cmd")
    assert [getattr(Cm, n).offset for n, _ in Cm._fields_] == [0, 8, 16, 20]
    assert plan.RECORD_DTYPE == pd.RECORD_DTYPE and plan.RECORD_DTYPE.itemsize == 16
    p = plan.plan_params()
    assert (p.v_max, p.w_max) == (0.6, 1.3)                            # navigate.cpp:33-34
    assert (p.horizon, p.robot_radius, p.w_goal, p.w_clear, p.w_speed, p.clear_cap) == (2.0, 0.3, 1.0, 0.5, 0.1, 1.0)
    assert (p.n_v, p.n_w, p.steps, p.reserved) == (3, 11, 20, 0)
    assert plan.plan_params(n_w=5).n_w == 5
    with pytest.raises(AttributeError):
        plan.plan_params(nw=5)
    consts = dict(re.findall(r"#define (JN_[A-Z_0-9]+) (\d+)", text))
    assert (plan.FAR, plan.MAX_RADIUS, plan.MAX_BATCH, plan.OK, plan.BLOCKED) == tuple(
        int(consts[k]) for k in ("JN_CLEARANCE_FAR", "JN_CLEARANCE_MAX_RADIUS", "JN_PLAN_MAX_BATCH", "JN_PLAN_OK", "JN_PLAN_BLOCKED"))
    assert (plan.FAR, plan.OK, plan.BLOCKED) == (pd.FAR, pd.OK, pd.BLOCKED) == (65535, 0, 1)
    assert plan.MAX_CELLS == costmap.MAX_CELLS == 512
    assert "GUESSES" in text and "tuned" in text and "SELF-REFERENTIAL" in text and "navigate.cpp:33-34" in text


BAD_PARAMS = [dict(v_max=0.0), dict(v_max=-0.6), dict(v_max=float("nan")), dict(v_max=float("inf")), dict(w_max=0.0), dict(w_max=float("nan")),
              dict(horizon=0.0), dict(horizon=float("inf")), dict(robot_radius=-0.1), dict(robot_radius=float("nan")),
              dict(robot_radius=0.05 * 255.5), dict(w_goal=-1.0), dict(w_goal=float("nan")), dict(w_clear=-1.0), dict(w_clear=float("inf")),
              dict(w_speed=-1.0), dict(clear_cap=-1.0), dict(clear_cap=float("nan")), dict(n_v=0), dict(n_v=17), dict(n_w=0), dict(n_w=2),
              dict(n_w=10), dict(n_w=67), dict(n_w=-1), dict(steps=0), dict(steps=129), dict(reserved=1)]


def test_invalid_arguments_are_refused_before_the_device_is_touched(jn):
    """Every check comes ahead of hipSetDevice: on a machine without a GPU these calls still say JN_ERR_INVALID, not JN_ERR_NO_DEVICE."""
    from jackal_navigation_amd import plan, _lib
    L = plan._bind()
    INV = _lib.JN_ERR_INVALID
    h = C.c_void_p()
    for kw in BAD_PARAMS:
        assert L.jn_plan_create(C.byref(plan.plan_params(**kw)), 0.05, 256, 256, 1, 0, C.byref(h)) == INV, kw
        assert not h.value
        assert L.jn_plan_templates(C.byref(plan.plan_params(**kw)), None, None, None) == (_lib.JN_OK if "robot_radius" in kw and kw["robot_radius"] > 0 else INV), kw
    good = plan.plan_params()
    for res, cx, cy, mb in ((0.0, 256, 256, 1), (-0.05, 256, 256, 1), (float("nan"), 256, 256, 1), (float("inf"), 256, 256, 1), (0.05, 0, 256, 1),
                            (0.05, 513, 256, 1), (0.05, 256, 0, 1), (0.05, 256, 513, 1), (0.05, 256, 256, 0), (0.05, 256, 256, -1),
                            (0.05, 256, 256, plan.MAX_BATCH + 1), (0.001, 256, 256, 1)):                 # the last: robot_radius / resolution > 255
        assert L.jn_plan_create(C.byref(good), res, cx, cy, mb, 0, C.byref(h)) == INV, (res, cx, cy, mb)
    assert L.jn_plan_create(None, 0.05, 256, 256, 1, 0, C.byref(h)) == INV
    assert L.jn_plan_create(C.byref(good), 0.05, 256, 256, 1, 0, None) == INV
    assert L.jn_plan_templates(None, None, None, None) == INV
    # the clearance transform
    p = 4096                                                           # never dereferenced
    for args in ((1, None, 8, 8, 0, 1, p), (1, p, 8, 8, 0, 1, None), (0, p, 8, 8, 0, 1, p), (-1, p, 8, 8, 0, 1, p), (plan.MAX_BATCH + 1, p, 8, 8, 0, 1, p),
                 (1, p, 0, 8, 0, 1, p), (1, p, 513, 8, 0, 1, p), (1, p, 8, 0, 0, 1, p), (1, p, 8, 513, 0, 1, p), (1, p, 8, 8, 2, 1, p), (1, p, 8, 8, -1, 1, p),
                 (1, p, 8, 8, 0, 0, p), (1, p, 8, 8, 0, 256, p), (1, p, 8, 8, 0, -3, p)):
        assert L.jn_clearance(0, *args) == INV, args
    # handle-bound calls: no handle (the checks that need one live in the GPU tests)
    org = (C.c_double * 2)(0.0, 0.0)
    pose = (plan.Pose2D * 1)(plan.Pose2D(0, 0, 0))
    rec = np.zeros(33, plan.RECORD_DTYPE); cmd = plan.PlanCmd(); goal = (C.c_double * 2)(1.0, 0.0)
    assert L.jn_plan_evaluate(None, 1, p, C.byref(org), pose, rec.ctypes.data) == INV
    assert L.jn_plan_command(None, 1, p, C.byref(org), pose, C.addressof(goal), C.addressof(cmd), None) == INV
    L.jn_plan_destroy(None)                                            # a no-op
    # the chooser
    ok = (C.byref(good), 0.05, rec.ctypes.data, C.byref(pose[0]), C.byref(goal), C.byref(cmd))
    assert L.jn_plan_choose(*ok) == _lib.JN_OK
    for k, bad in ((0, None), (1, 0.0), (1, float("nan")), (1, 0.001), (2, None), (3, None), (4, None), (5, None)):
        args = list(ok); args[k] = bad
        assert L.jn_plan_choose(*args) == INV, k
    for bad_pose in (plan.Pose2D(float("nan"), 0, 0), plan.Pose2D(0, float("inf"), 0), plan.Pose2D(0, 0, float("nan")), plan.Pose2D(0.05 * 2.0 ** 30 * 1.01, 0, 0)):
        assert L.jn_plan_choose(C.byref(good), 0.05, rec.ctypes.data, C.byref(bad_pose), C.byref(goal), C.byref(cmd)) == INV
    for bad_goal in ((float("nan"), 0.0), (0.0, float("-inf")), (0.0, 0.05 * 2.0 ** 30 * 1.01)):
        assert L.jn_plan_choose(C.byref(good), 0.05, rec.ctypes.data, C.byref(pose[0]), C.byref((C.c_double * 2)(*bad_goal)), C.byref(cmd)) == INV


def test_create_without_a_device_fails_loudly(jn):
    from jackal_navigation_amd import plan, _lib
    from jackal_navigation_amd.device import device_count
    if device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.JnError) as e:
        plan.Plan(plan.plan_params(), 0.05, 256, 256)
    assert e.value.status == _lib.JN_ERR_NO_DEVICE
    with pytest.raises(_lib.JnError) as e:
        plan.clearance(np.zeros((4, 4), np.int8), 2)
    assert e.value.status == _lib.JN_ERR_NO_DEVICE


def test_twist_message_fields(jn):
    from jackal_navigation_amd import plan
    m = plan.twist_message(plan.PlanCmd(0.4, -0.26, 14, plan.OK))
    assert m == {"linear": {"x": 0.4, "y": 0.0, "z": 0.0}, "angular": {"x": 0.0, "y": 0.0, "z": -0.26}}
    z = plan.twist_message(plan.PlanCmd(0.0, 0.0, -1, plan.BLOCKED))
    assert z["linear"]["x"] == 0.0 and z["angular"]["z"] == 0.0


# ---- host code of the library against the checker, bit for bit ----

def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


TEMPLATE_SETS = [dict(), dict(n_w=1), dict(steps=1), dict(n_v=1, n_w=1, steps=1), dict(n_v=16, n_w=65, steps=128), dict(n_w=65, w_max=1e-300),
                 dict(n_v=2, n_w=3, steps=7, horizon=0.37, v_max=0.123, w_max=2.9), dict(n_w=5, horizon=100.0, w_max=3.0)]


@pytest.mark.parametrize("kw", TEMPLATE_SETS, ids=[str(i) for i in range(len(TEMPLATE_SETS))])
def test_templates_equal_libm_bit_for_bit(jn, kw):
    """The library's sines and cosines are the C library's, as Python's math.sin / math.cos are: equality on the bits, w = 0 (the middle
    candidate, and n_w = 1), the smallest non-zero w, one step, the largest set."""
    from jackal_navigation_amd import plan
    p = plan.plan_params(**kw)
    v, w, xy = plan.templates(p)
    wv, ww, wxy = pd.templates(p)
    assert v.shape == (p.n_v * p.n_w,) and xy.shape == (p.n_v * p.n_w, p.steps, 2)
    assert np.array_equal(_bits(v), _bits(wv)) and np.array_equal(_bits(w), _bits(ww)) and np.array_equal(_bits(xy), _bits(wxy))
    m = (p.n_w - 1) // 2
    assert (w.reshape(p.n_v, p.n_w)[:, m] == 0.0).all() and (xy.reshape(p.n_v, p.n_w, p.steps, 2)[:, m, :, 1] == 0.0).all()
    if p.n_w > 1:
        assert w[0] == -p.w_max and w[p.n_w - 1] == p.w_max and w[m + 1] > 0 and np.array_equal(w[:p.n_w], -w[:p.n_w][::-1])
        assert (xy.reshape(p.n_v, p.n_w, p.steps, 2)[:, m + 1:, :, 1] >= 0).all()       # positive w turns left: y >= 0 (1 - cos is 0 for a tiny angle)
    assert v[-1] == p.v_max and (np.diff(v.reshape(p.n_v, p.n_w)[:, 0]) > 0).all()
    # either output alone
    L = plan._bind()
    only = np.empty_like(w)
    assert L.jn_plan_templates(C.byref(p), None, only.ctypes.data, None) == 0 and np.array_equal(_bits(only), _bits(w))


def _records(p, rows):
    rec = np.zeros(p.n_v * p.n_w, pd.RECORD_DTYPE)
    rec["t_end"], rec["t_hit"], rec["min_d2"], rec["last_cell"] = p.steps, 0, pd.FAR, -1          # everything blocked at step 0
    for k, row in rows.items():
        rec[k] = row
    return rec


def _both(plan, p, res, rec, pose, goal):
    got = plan.choose(p, res, rec, pose, goal)
    want = pd.choose(p, res, rec, pose, goal)
    assert (got.candidate, got.status) == want[2:], (got.candidate, got.status, want)
    assert np.array_equal(_bits([got.v, got.w]), _bits(want[:2]))
    return got


def test_chooser_on_hand_made_records(jn):
    from jackal_navigation_amd import plan
    p = plan.plan_params()
    T, res = p.steps, 0.05
    free = (T, T, 400, 7)
    # all blocked -> (0, 0), candidate -1, the blocked status
    c = _both(plan, p, res, _records(p, {}), (0, 0, 0), (5.0, 0.0))
    assert (c.v, c.w, c.candidate, c.status) == (0.0, 0.0, -1, plan.BLOCKED)
    # a candidate that hit nothing but has no step on the grid (t_end = 0) is not admissible
    c = _both(plan, p, res, _records(p, {5: (0, T, pd.FAR, -1)}), (0, 0, 0), (5.0, 0.0))
    assert c.status == plan.BLOCKED
    # a tie goes to the lowest k: the two mirror-image arcs of the slowest speed with the goal on the axis
    c = _both(plan, p, res, _records(p, {3: free, 7: free}), (0, 0, 0), (5.0, 0.0))
    assert c.candidate == 3 and c.w < 0
    c = _both(plan, p, res, _records(p, {7: free, 3: free, 4: free, 6: free}), (0, 0, 0), (5.0, 0.0))
    assert c.candidate == 4                                           # the straighter pair is nearer the goal; of it, the lower k
    # everything free and the goal straight ahead: the fastest w = 0 candidate
    allfree = _records(p, {k: free for k in range(p.n_v * p.n_w)})
    c = _both(plan, p, res, allfree, (0, 0, 0), (5.0, 0.0))
    assert c.candidate == 2 * p.n_w + 5 and (c.v, c.w) == (p.v_max, 0.0) and c.status == plan.OK
    # the goal to the left: a left turn (w > 0); behind a pose turned by pi: the same choice as ahead of the zero pose
    assert _both(plan, p, res, allfree, (0, 0, 0), (1.0, 1.0)).w > 0
    assert _both(plan, p, res, allfree, (1.0, -2.0, math.pi), (-4.0, -2.0)).candidate == 2 * p.n_w + 5
    # min_d2 = FAR is a number like any other (sqrt(65535) cells, then the cap); clear_cap active: 400 and 10000 cells^2 score the same
    a = _records(p, {16: (T, T, pd.FAR, 3), 5: (T, T, 10000, 3)})
    b = _records(p, {16: (T, T, 400, 3), 5: (T, T, 10000, 3)})
    assert math.sqrt(400.0) * res == p.clear_cap
    assert _both(plan, p, res, a, (0, 0, 0), (5.0, 0.0)).candidate == _both(plan, p, res, b, (0, 0, 0), (5.0, 0.0)).candidate == 16
    # below the cap clearance counts: with a heavy w_clear the slow candidate in the open beats the fast one that grazes a wall
    pc = plan.plan_params(w_clear=50.0)
    c = _both(plan, pc, res, _records(pc, {27: (T, T, 37, 3), 5: (T, T, 399, 3)}), (0, 0, 0), (5.0, 0.0))
    assert c.candidate == 5
    # an arc that leaves the grid early is scored at its last step on it
    c = _both(plan, p, res, _records(p, {27: (1, T, 400, 3), 5: (T, T, 400, 3)}), (0, 0, 0), (5.0, 0.0))
    assert c.candidate == 5
    # random records, poses and goals
    rng = np.random.default_rng(11)
    for trial in range(200):
        q = plan.plan_params(n_v=int(rng.integers(1, 5)), n_w=int(rng.integers(0, 6)) * 2 + 1, steps=int(rng.integers(1, 30)),
                             w_clear=float(rng.uniform(0, 3)), w_speed=float(rng.uniform(0, 1)), clear_cap=float(rng.uniform(0, 2)))
        K = q.n_v * q.n_w
        rec = np.zeros(K, pd.RECORD_DTYPE)
        rec["t_end"] = rng.integers(0, q.steps + 1, K)
        rec["t_hit"] = np.where(rng.random(K) < 0.5, q.steps, rng.integers(0, q.steps + 1, K))
        rec["min_d2"] = np.where(rng.random(K) < 0.2, pd.FAR, rng.integers(1, 3000, K))
        rec["last_cell"] = rng.integers(-1, 100, K)
        pose = (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5)), float(rng.uniform(-7, 7)))
        _both(plan, q, float(rng.choice([0.05, 0.1, 0.031])), rec, pose, (float(rng.uniform(-9, 9)), float(rng.uniform(-9, 9))))


# ---- the definition itself, on cases small enough to do by hand ----

def test_clearance_of_one_obstacle_cell_is_the_table_of_squares():
    g = np.zeros((31, 41), np.int8)
    g[12, 30] = 100
    ys, xs = np.mgrid[0:31, 0:41]
    table = (xs - 30) ** 2 + (ys - 12) ** 2
    for R in (1, 2, 7, 20, 255):
        want = np.where(table <= R * R, table, pd.FAR).astype(np.uint16)
        d2 = pd.clearance(g, R)
        assert d2.dtype == np.uint16 and np.array_equal(d2, want), R
        assert d2[12, 30] == 0
    assert sorted(np.unique(pd.clearance(g, 1)).tolist()) == [0, 1, pd.FAR] and int((pd.clearance(g, 1) == 1).sum()) == 4


def test_clearance_radius_255_on_the_largest_grid():
    g = np.zeros((512, 512), np.int8)
    g[0, 0] = 100
    d2 = pd.clearance(g, 255)
    assert d2[0, 255] == 65025 and d2[255, 0] == 65025 and d2[0, 256] == pd.FAR and d2[180, 180] == 64800 and d2[181, 181] == pd.FAR
    assert int(d2[d2 != pd.FAR].max()) == 65025


def test_clearance_unknown_empty_full_and_values_that_are_not_obstacles():
    g = np.zeros((9, 13), np.int8)
    assert (pd.clearance(g, 5) == pd.FAR).all() and (pd.clearance(g, 5, 1) == pd.FAR).all()           # empty: all FAR
    assert (pd.clearance(np.full((9, 13), 100, np.int8), 3) == 0).all()                               # full: all 0
    u = np.full((9, 13), -1, np.int8)
    assert (pd.clearance(u, 3, 0) == pd.FAR).all() and (pd.clearance(u, 3, 1) == 0).all()
    g[4, 6] = -1; g[0, 0] = 100; g[8, 12] = 99; g[8, 0] = 50; g[0, 12] = -100
    off, on = pd.clearance(g, 4, 0), pd.clearance(g, 4, 1)
    assert off[4, 6] == pd.FAR and on[4, 6] == 0 and on[4, 8] == 4 and off[0, 0] == on[0, 0] == 0
    assert off[8, 12] == off[8, 0] == off[0, 12] == pd.FAR                                            # only 100 (and -1 when asked) count
    assert (on <= off).all()


def test_clearance_symmetries_monotonicity_and_both_brute_forces():
    rng = np.random.default_rng(4)
    for shape, dens, R in (((23, 37), 0.01, 9), ((40, 17), 0.2, 5), ((1, 50), 0.1, 60), ((50, 1), 0.1, 3), ((1, 1), 1.0, 1), ((30, 30), 0.003, 255)):
        g = np.where(rng.random(shape) < dens, 100, 0).astype(np.int8)
        g[rng.random(shape) < 0.1] = -1
        for unk in (0, 1):
            d2 = pd.clearance(g, R, unk)
            obst = pd.obstacles(g, unk)
            assert np.array_equal(pd._by_obstacle(obst, R), pd._by_offset(obst, R)) and np.array_equal(d2, pd._by_obstacle(obst, R))
            assert np.array_equal(d2 == 0, obst)
            assert np.array_equal(pd.clearance(g.T, R, unk), d2.T)                                   # transposed grid -> transposed field
            assert np.array_equal(pd.clearance(g[::-1, ::-1], R, unk), d2[::-1, ::-1])
            more = g.copy()
            more[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = 100
            assert (pd.clearance(more, R, unk) <= d2).all()                                          # an added obstacle never raises any d2
            if R < 255:
                assert (pd.clearance(g, R + 1, unk) <= d2).all()


def test_rollout_and_choice_by_hand():
    """A 40 x 40 grid of 0.1 m cells whose corner is (-1.05, -2.05) (the points below fall in the middle of cells): the robot at the origin
    looks along +x at a wall 2 m ahead."""
    from jackal_navigation_amd import plan
    p = plan.plan_params(n_v=2, n_w=3, steps=10, horizon=5.0, robot_radius=0.25)
    res, org = 0.1, (-1.05, -2.05)
    g = np.zeros((40, 40), np.int8)
    g[:, 30] = 100                                                     # x in [1.95, 2.05)
    d2 = pd.clearance(g, 10)
    assert pd.r2_of(p, res) == 6                                       # floor(2.5^2)
    rec = pd.rollout(p, res, d2, org, (0.0, 0.0, 0.0))
    # k = 4: v = 0.6, w = 0: x_t = 0.3 (s + 1).  d2 <= 6 from 2 cells away: cells 28.. -> x >= 1.8 -> step 5; before it the nearest is
    # step 4 at x = 1.5 (cell 25: 5 cells away)
    assert rec[4].tolist() == (10, 5, 25, 20 * 40 + 25)
    # k = 1: v = 0.3, w = 0: x_t = 0.15 (s + 1) reaches 1.5 at the last step and never hits
    assert rec[1].tolist() == (10, 10, 25, 20 * 40 + 25)
    best = pd.choose(p, res, rec, (0.0, 0.0, 0.0), (5.0, 0.0))
    assert best[3] == pd.OK and best[2] != 4 and rec[best[2]]["t_hit"] == 10
    # from outside the grid every candidate ends at step 0 and the robot is blocked
    out = pd.rollout(p, res, d2, org, (10.0, 0.0, 0.0))
    assert (out["t_end"] == 0).all() and (out["t_hit"] == 10).all() and (out["min_d2"] == pd.FAR).all() and (out["last_cell"] == -1).all()
    assert pd.choose(p, res, out, (10.0, 0.0, 0.0), (5.0, 0.0)) == (0.0, 0.0, -1, pd.BLOCKED)
    # turned by pi / 2 the robot drives along +y, off the grid's top edge (y = 1.95): 0.3 (s + 1) >= 1.95 at step 6
    up = pd.rollout(p, res, d2, org, (0.0, 0.0, math.pi / 2))
    assert up[4]["t_end"] == 6 and up[4]["t_hit"] == 10

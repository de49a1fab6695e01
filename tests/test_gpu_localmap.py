"""The odometry-fused local obstacle map (include/jn_localmap.h) on the GPU against its scalar definition (tests/localmap_def.py),
everything bit for bit: the frames' counts, the log-odds state and the grid, through updates, recentres and resets; the anchor in
jn_subpix_costmap; a driving scene on exact disparities; real matcher output."""
import ctypes as C
import math

import numpy as np
import pytest

import ground_def as gd
import localmap_def as ld
import subpix_def as sd
from localmap_check import as_format, generic_poses, gpu_update, random_q, same_state, step, tweak_w0

pytestmark = pytest.mark.gpu

FORMATS = (ld.F32, ld.I16, ld.I16_SUB)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W,H,n,cx,cy,res", [(8, 8, 1, 1, 1, 50.0), (200, 37, 3, 7, 13, 0.31), (1280, 720, 2, 256, 256, 0.05), (1919, 1079, 1, 512, 512, 0.03),
                                             (321, 180, 33, 1, 64, 0.2), (64, 48, 2, 64, 1, 0.2)])
def test_counts_and_state_equal_the_definition(jn, fmt, W, H, n, cx, cy, res):
    from jackal_navigation_amd import localmap, node
    rng = np.random.default_rng(1000 * fmt + W + n)
    sp = tweak_w0(node.scan_params(W, H))
    sp.crop_offset_x, sp.crop_offset_y = 5, 3
    p = localmap.localmap_params(fmt, cells_x=cx, cells_y=cy, resolution=res, min_hits=2, min_floor=2)
    maps = as_format(random_q(rng, n, H, W), fmt)
    poses = generic_poses(rng, n) if cx * cy > 1 else [(1.0, 25.0, 0.3)]            # the one cell is [0, 50) x [0, 50)
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=n) as m:
        same_state(m, ref, "new handle")
        o, f = step(m, ref, sp, poses, maps, (fmt, W, H))
        assert int(o.sum()) + int(f.sum()) > 0 and (W <= 8 or (o.sum() > 0 and f.sum() > 0))
        assert (ref.L != 0).any()
        # the same batch once more, with the counts not asked for
        from jackal_navigation_amd.device import DeviceArray
        dD = DeviceArray.from_numpy(maps)
        m.update(sp, poses, dD.ptr, W, H)
        ref.update(sp, poses, maps)
        same_state(m, ref, "no count outputs")
        dD.free()


@pytest.mark.parametrize("fmt", FORMATS)
def test_all_invalid_all_floor_all_obstacle(jn, fmt):
    from jackal_navigation_amd import localmap, node
    W, H = 320, 180
    p = localmap.localmap_params(fmt, cells_x=200, cells_y=120)
    fill = {ld.F32: -10.0, ld.I16: -1, ld.I16_SUB: -16}[fmt]
    invalid = np.full((2, H, W), fill, localmap.FORMAT_DTYPES[fmt])
    if fmt == ld.F32:
        invalid[1, ::3] = np.nan; invalid[1, 1::3] = np.inf
    rng = np.random.default_rng(3)
    maps = as_format(rng.integers(200, 900, (2, H, W)), fmt)
    poses = [(0.2, -0.1, 0.3), (0.0, 0.0, -0.2)]
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=2) as m:
        o, f = step(m, ref, node.scan_params(W, H), poses, invalid, "invalid")
        assert not o.any() and not f.any() and not ref.L.any()
        sp = node.scan_params(W, H); sp.gp_height_thresh = 1e9                      # every point is on the ground model
        o, f = step(m, ref, sp, poses, maps, "floor")
        assert not o.any() and f.sum() > 0 and (ref.L <= 0).all() and (ref.L < 0).any()
        sp = node.scan_params(W, H); sp.gp_height_thresh = -1e9                     # no point is
        o, f = step(m, ref, sp, poses, maps, "obstacle")
        assert not f.any() and o.sum() > 0 and (ref.L > 0).any()


def test_counts_saturate_at_65535(jn):
    """One 1 km cell collects a whole 640x480 frame: 307200 pixels, stored as 65535, as obstacle and as floor; 57000 stay 57000."""
    from jackal_navigation_amd import localmap, node
    W, H = 640, 480
    p = localmap.localmap_params(ld.I16_SUB, cells_x=1, cells_y=1, resolution=1000.0)
    maps = np.full((2, H, W), 40 * 16 + 5, np.int16)
    maps[1, :100] = -16
    maps[1, 100:, 150:] = -16
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=2) as m:
        assert ref.g0 == (0, 0)                                                      # the cell is [0, 1000) x [0, 1000)
        for thresh, k in ((-1e9, 0), (1e9, 1)):
            sp = node.scan_params(W, H); sp.gp_height_thresh = thresh
            sp.XT[0], sp.XT[1] = 500.0, 500.0                                        # the camera in the middle of the cell
            of = step(m, ref, sp, [(0, 0, 0), (0, 0, 0)], maps, thresh)
            assert of[k][:, 0, 0].tolist() == [65535, 57000] and not of[1 - k].any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_anchor_in_the_subpixel_costmap(jn, fmt):
    """Zero pose, the window's origin equal to a costmap's: dObst is jn_subpix_costmap's dHits, bit for bit (device against device)."""
    from jackal_navigation_amd import costmap, localmap, node, subpix
    from jackal_navigation_amd.device import DeviceArray
    W, H, n = 641, 353, 3
    rng = np.random.default_rng(77 + fmt)
    sp = tweak_w0(node.scan_params(W, H))
    sp.crop_offset_x, sp.crop_offset_y = 2, 9
    maps = as_format(random_q(rng, n, H, W), fmt)
    p = localmap.localmap_params(fmt, cells_x=128, cells_y=128)
    with localmap.LocalMap(p, max_batch=n) as m:
        m.recenter(64 * 0.05, 0.0)                                                    # g0 = (0, -64): origin (0.0, -3.2), the costmap's default
        w = m.window()
        cp = costmap.costmap_params(origin_x=w.origin[0], origin_y=w.origin[1], resolution=p.resolution, cells_x=128, cells_y=128)
        assert w.g0 == (0, -64) and (cp.origin_x, cp.origin_y) == (0.0, -3.2) == (costmap.costmap_params().origin_x, costmap.costmap_params().origin_y)
        o, f = gpu_update(m, sp, [(0.0, 0.0, 0.0)] * n, maps)
    dD = DeviceArray.from_numpy(maps)
    bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    hits = DeviceArray((n, 128, 128), np.uint16); grid = DeviceArray((n, 128, 128), np.int8)
    subpix.subpix_costmap(sp, cp, subpix.subpix_params(fmt), n, dD.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr)
    assert np.array_equal(o, hits.numpy()) and o.sum() > 0 and f.sum() > 0


def _hit_miss_nothing(sp, W, H):
    """Three I16_SUB maps for a one-cell window: a wall 2 m ahead (obstacle pixels: a hit), the floor (a miss), nothing valid."""
    wall = sd.wall_q(sp, W, H, 2.0)[0].astype(np.int16)
    fl = np.rint(16.0 * gd.floor_disparity(sp, list(sp.XR), list(sp.XT), W, H))
    floor = np.where((fl >= 32) & (fl < 30000), fl, -16).astype(np.int16)
    return wall, floor, np.full((H, W), -16, np.int16)


def test_fusion_sequence_clamps_thresholds_and_order(jn):
    from jackal_navigation_amd import localmap, node
    W, H = 160, 90
    sp = node.scan_params(W, H)
    A, B, N = _hit_miss_nothing(sp, W, H)
    p = localmap.localmap_params(ld.I16_SUB, cells_x=1, cells_y=1, resolution=100.0)
    z = (0.0, 0.0, 0.0)
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=8) as m:
        seen = []
        for k, mp in enumerate([A] * 5 + [N] + [B] * 26 + [N, A]):
            step(m, ref, sp, [z], mp[None], k)
            seen.append((int(ref.L[0, 0]), int(ref.grid()[0, 0])))
        L = [s[0] for s in seen]
        assert L[:6] == [4, 8, 12, 16, 16, 16]                                       # + l_hit, the clamp at l_max, nothing seen
        assert L[6:32] == list(range(15, -9, -1)) + [-8, -8]                        # - l_miss down to the clamp at l_min
        assert L[32:] == [-8, -4]
        for l, g in seen:
            assert g == (100 if l >= 4 else (0 if l <= -2 else -1))
        assert {(4, 100), (3, -1), (-1, -1), (-2, 0)} <= set(seen)                  # both thresholds from both sides
        # order inside a call: from 14, [hit, miss] ends at 15 and [miss, hit] at 16
        p7 = localmap.localmap_params(ld.I16_SUB, cells_x=1, cells_y=1, resolution=100.0, l_hit=7)
        for order, want in (((A, B), 15), ((B, A), 16)):
            r7 = ld.Map(p7)
            with localmap.LocalMap(p7, max_batch=4) as m7:
                step(m7, r7, sp, [z, z], np.stack([A, A]), "to 14")
                assert int(r7.L[0, 0]) == 14
                step(m7, r7, sp, [z, z], np.stack(order), "order")
                assert int(m7.read()[0][0, 0]) == want


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_call_of_n_frames_equals_n_calls(jn, fmt):
    from jackal_navigation_amd import localmap, node
    W, H, n = 320, 180, 6
    rng = np.random.default_rng(40 + fmt)
    sp = node.scan_params(W, H)
    maps = as_format(random_q(rng, n, H, W), fmt)
    poses = generic_poses(rng, n)
    p = localmap.localmap_params(fmt, cells_x=96, cells_y=160, min_hits=1, min_floor=1, l_hit=5, l_miss=3, l_min=-7, l_max=9)
    with localmap.LocalMap(p, max_batch=n) as a, localmap.LocalMap(p, max_batch=1) as b:
        oa, fa = gpu_update(a, sp, poses, maps)
        for k in range(n):
            ob, fb = gpu_update(b, sp, poses[k:k + 1], maps[k:k + 1])
            assert np.array_equal(ob[0], oa[k]) and np.array_equal(fb[0], fa[k])
        La, Lb = a.read(), b.read()
        assert np.array_equal(La[0], Lb[0]) and np.array_equal(La[1], Lb[1])
        assert (La[0] == 9).any() and (La[0] == -7).any()                            # both clamps were reached on the way
        ref = ld.Map(p); ref.update(sp, poses, maps)
        same_state(a, ref)


@pytest.mark.parametrize("fmt", FORMATS)
def test_equivariance_under_whole_cell_shifts(jn, fmt):
    """resolution a power of two, theta = 0: shifting every pose and the window by whole cells changes nothing in window coordinates."""
    from jackal_navigation_amd import localmap, node
    W, H, n = 320, 180, 3
    rng = np.random.default_rng(60 + fmt)
    sp = node.scan_params(W, H)
    maps = as_format(random_q(rng, n, H, W), fmt)
    p = localmap.localmap_params(fmt, cells_x=200, cells_y=200, resolution=0.0625)
    base = [(0.0, 0.0, 0.0), (0.25, -0.125, 0.0), (0.5, 0.0625, 0.0)]
    outs = []
    for kx, ky in ((0, 0), (37, -91), (-1000, 4096)):
        sx, sy = kx * 0.0625, ky * 0.0625
        poses = [(x + sx, y + sy, t) for x, y, t in base]
        ref = ld.Map(p)
        with localmap.LocalMap(p, max_batch=n) as m:
            m.recenter(sx, sy); ref.recenter(sx, sy)
            assert ref.g0 == (kx - 100, ky - 100)
            o, f = step(m, ref, sp, poses, maps, (kx, ky))
            outs.append((o, f) + m.read())
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b)
    assert outs[0][0].sum() > 0 and outs[0][1].sum() > 0


def test_recentre_keeps_the_overlap_and_clears_what_enters(jn):
    from jackal_navigation_amd import localmap, node
    W, H, n = 320, 180, 2
    rng = np.random.default_rng(90)
    sp = node.scan_params(W, H)
    maps = as_format(random_q(rng, n, H, W), ld.I16_SUB)
    p = localmap.localmap_params(ld.I16_SUB, cells_x=100, cells_y=60, resolution=0.1, min_hits=1, min_floor=1)
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=n) as m:
        step(m, ref, sp, [(0.0, 0.0, 0.0), (0.3, 0.2, 1.0)], maps, "fill")
        before = ref.L.copy()
        assert (before != 0).sum() > 200
        m.recenter(1.23, -0.77); ref.recenter(1.23, -0.77)                          # +12 cells in x, -8 in y
        same_state(m, ref, "overlap")
        assert ref.g0 == (12 - 50, -8 - 30) and np.array_equal(ref.L[8:, :88], before[:52, 12:]) and not ref.L[:8].any() and not ref.L[:, 88:].any()
        m.recenter(1.23, -0.77); same_state(m, ref, "no move")
        step(m, ref, sp, [(1.2, -0.7, -2.0), (1.0, -1.0, 0.5)], maps, "update in the moved window")
        # many small moves: the window travels several of its own widths and comes back; negative global indices on the way
        x = 1.23
        for k in range(70):
            x -= 0.37
            m.recenter(x, -0.77); ref.recenter(x, -0.77)
            if k % 9 == 0:
                step(m, ref, sp, [(x, -0.7, 0.1 * k)], maps[:1], ("walk", k))
        assert ref.g0[0] < -250
        same_state(m, ref, "walked")
        m.recenter(0.0, -123.456); ref.recenter(0.0, -123.456)                      # a move larger than the window empties it
        same_state(m, ref, "far")
        assert not m.read()[0].any() and ref.g0[1] == -1235 - 30
        step(m, ref, sp, [(0.0, -123.0, 0.7)], maps[:1], "far update")
        m.reset(); ref.reset()
        same_state(m, ref, "reset")
        assert not m.read()[0].any() and m.window().g0 == (-50, -30)


def test_follow_is_a_host_policy_on_top_of_recentre(jn):
    from jackal_navigation_amd import localmap
    p = localmap.localmap_params(ld.F32, cells_x=64, cells_y=64, resolution=0.1)
    with localmap.LocalMap(p) as m:
        assert m.window().g0 == (-32, -32)
        assert not m.follow((0.95, -0.95, 0.0), 10) and m.window().g0 == (-32, -32)  # cell (9, -10): inside the margin
        assert m.follow(localmap.Pose2D(1.15, 0.0, 0.0), 10) and m.window().g0 == (11 - 32, -32)
        assert not m.follow((1.15, 0.0, 0.0), 0)
        assert m.follow((1.15, -0.11, 0.0), 0) and m.window().g0 == (11 - 32, -2 - 32)


def test_invalid_calls_on_a_live_handle(jn):
    from jackal_navigation_amd import localmap, node, _lib
    from jackal_navigation_amd.device import DeviceArray
    W, H = 64, 48
    sp = node.scan_params(W, H)
    p = localmap.localmap_params(ld.I16, cells_x=32, cells_y=32)
    dD = DeviceArray.from_numpy(np.full((2, H, W), 20, np.int16))
    L = localmap._bind()
    with localmap.LocalMap(p, max_batch=2) as m:
        m.update(sp, [(0, 0, 0), (0, 0, 0)], dD.ptr, W, H)
        state = m.read()
        ok = (localmap.Pose2D * 3)(localmap.Pose2D(0, 0, 0), localmap.Pose2D(0, 0, 0), localmap.Pose2D(0, 0, 0))
        S = C.byref(sp)
        for args in ((None, 1, ok, dD.ptr, W, H), (S, 0, ok, dD.ptr, W, H), (S, 3, ok, dD.ptr, W, H), (S, -1, ok, dD.ptr, W, H), (S, 1, None, dD.ptr, W, H),
                     (S, 1, ok, None, W, H), (S, 1, ok, dD.ptr, 0, H), (S, 1, ok, dD.ptr, W, 0)):
            assert L.jn_localmap_update(m._h, *args, None, None) == _lib.JN_ERR_INVALID, args
        for bad in ((float("nan"), 0, 0), (0, float("inf"), 0), (0, 0, float("nan")), (0, 0, float("inf")), (0.05 * 2.0 ** 30 * 1.01, 0, 0),
                    (0, -0.05 * 2.0 ** 30 * 1.01, 0)):
            with pytest.raises(_lib.JnError) as e:
                m.update(sp, [(0, 0, 0), bad], dD.ptr, W, H)
            assert e.value.status == _lib.JN_ERR_INVALID
        for bad in ((float("nan"), 0.0), (0.0, float("-inf")), (0.05 * 2.0 ** 30 * 1.01, 0.0)):
            with pytest.raises(_lib.JnError) as e:
                m.recenter(*bad)
            assert e.value.status == _lib.JN_ERR_INVALID
        assert L.jn_localmap_read(m._h, None, None) == _lib.JN_ERR_INVALID
        after = m.read()
        assert np.array_equal(state[0], after[0]) and np.array_equal(state[1], after[1]) and m.window().g0 == (-16, -16)
        m.update(sp, [(0.05 * 2.0 ** 30, 0, 0)], dD.ptr, W, H)                       # the limit itself is admitted
        dL = DeviceArray((32, 32), np.int16)
        m.read_device(dL.ptr, None)                                                   # either output alone
        assert np.array_equal(dL.numpy(), m.read()[0])


def drive_scene(sp, W, H):
    """Exact disparities (1/16 pixel) of the floor, and of the floor with a wall 2 m ahead across the middle columns."""
    fl = np.rint(16.0 * gd.floor_disparity(sp, list(sp.XR), list(sp.XT), W, H))
    floor = np.where((fl >= 32) & (fl < 30000), fl, -16).astype(np.int16)
    wq = sd.wall_q(sp, W, H, 2.0)[0]
    wall = floor.copy()
    cols = slice(W // 2 - 50, W // 2 + 50)
    wall[:, cols] = np.where(wq[:, cols] > floor[:, cols], wq[:, cols], floor[:, cols])     # the nearer surface is the one seen
    return floor, wall


def test_a_wall_is_remembered_after_the_robot_turns_away(jn):
    from jackal_navigation_amd import localmap, node
    W, H = 320, 180
    sp = node.scan_params(W, H)
    floor, wall = drive_scene(sp, W, H)
    p = localmap.localmap_params(ld.I16_SUB)
    ref = ld.Map(p)
    with localmap.LocalMap(p, max_batch=2) as m:
        o, f = step(m, ref, sp, [(0.0, 0.0, 0.0)] * 2, np.stack([wall, wall]), "facing the wall")
        wall_cells = o[0] >= p.min_hits
        front = (f[0] >= p.min_floor) & ~wall_cells
        assert wall_cells.sum() >= 10 and front.sum() > 500
        g = m.read()[1]
        assert (g[wall_cells] == 100).all() and (g[front] == 0).all()
        for k, theta in enumerate((1.7, 2.0, 2.3, -2.5, -1.9)):                         # turned away: the wall is behind the field of view
            o2, f2 = step(m, ref, sp, [(0.0, 0.0, theta)], floor[None], ("turned", theta))
            assert not (o2[0] >= p.min_hits).any() and not (f2[0][wall_cells] >= p.min_floor).any()
        L, g = m.read()
        assert (g[wall_cells] == 100).all() and (L[wall_cells] == 2 * p.l_hit).all() and (g[front] == 0).all()
        assert (g == 0).sum() > 3 * front.sum() // 2                                    # and the floor seen meanwhile is free


def test_a_phantom_is_cleared_by_floor_sightings(jn):
    """A blob present in frame 0 only: its cells fall below occ_thresh after ceil((L0 - occ_thresh + 1) / l_miss) sightings of the floor there."""
    from jackal_navigation_amd import localmap, node
    W, H = 320, 180
    sp = node.scan_params(W, H)
    floor, _ = drive_scene(sp, W, H)
    blob = floor.copy()
    blob[60:100, 140:170] = sd.wall_q(sp, W, H, 1.5)[0][60:100, 140:170]
    p = localmap.localmap_params(ld.I16_SUB, l_hit=9, l_miss=2)
    ref = ld.Map(p)
    z = (0.0, 0.0, 0.0)
    with localmap.LocalMap(p, max_batch=1) as m:
        o, f = step(m, ref, sp, [z], blob[None], "blob")
        o1, f1 = ld.counts(sp, p, ref.g0, z, floor)
        cells = (o[0] >= p.min_hits) & (f1 >= p.min_floor) & (o1 < p.min_hits)         # phantom cells whose floor the next frames see
        assert cells.sum() >= 3
        L0 = p.l_hit
        need = math.ceil((L0 - p.occ_thresh + 1) / p.l_miss)
        assert need == 3
        for k in range(1, need + 1):
            step(m, ref, sp, [z], floor[None], ("floor", k))
            L, g = m.read()
            assert (L[cells] == L0 - k * p.l_miss).all()
            assert ((g[cells] == 100).all() and k < need) or ((g[cells] != 100).all() and k == need), k


def test_real_matcher_output_elas_and_sgm(jn):
    """ELAS's float dD1 and the SGM mode's 1/16-pixel map, straight from the matchers' device buffers after the synchronous calls."""
    from jackal_navigation_amd import localmap, node
    from jackal_navigation_amd.device import DeviceArray
    W, H, B = 320, 180, 2
    sp = node.scan_params(W, H)
    pairs = [node.synth_pair(W, H, 40, 500 + t) for t in range(B)]
    dL = DeviceArray.from_numpy(np.stack([a for a, _ in pairs])); dR = DeviceArray.from_numpy(np.stack([b for _, b in pairs]))
    poses = [(0.0, 0.0, 0.0), (0.1, 0.05, 0.2)]
    d1 = DeviceArray((B, H, W), np.float32); d2 = DeviceArray((B, H, W), np.float32)
    with jn.Elas(jn.Elas.parameters(0), W, H, max_batch=B) as e:
        e.process_batch(B, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr)
    dd = DeviceArray((B, H, W), np.int16)
    with jn.Sgm(jn.Sgm.parameters(num_disparities=64, subpixel=1), W, H, max_batch=B) as s:
        s.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd.ptr)
    for fmt, dev in ((ld.F32, d1), (ld.I16_SUB, dd)):
        p = localmap.localmap_params(fmt)
        ref = ld.Map(p)
        maps = dev.numpy()
        if fmt == ld.I16_SUB:
            assert (maps[maps > 0] % 16 != 0).any()
        with localmap.LocalMap(p, max_batch=B) as m:
            dO = DeviceArray((B, p.cells_y, p.cells_x), np.uint16); dF = DeviceArray((B, p.cells_y, p.cells_x), np.uint16)
            m.update(sp, poses, dev.ptr, W, H, dO.ptr, dF.ptr)
            wo, wf = ref.update(sp, poses, maps)
            assert np.array_equal(dO.numpy(), wo) and np.array_equal(dF.numpy(), wf)
            assert int(wo.sum()) + int(wf.sum()) > 1000
            same_state(m, ref, fmt)
            assert (ref.L != 0).any()


def test_the_same_sequence_twice_gives_the_same_bytes(jn):
    from jackal_navigation_amd import localmap, node
    W, H, n = 640, 360, 4
    rng = np.random.default_rng(123)
    sp = node.scan_params(W, H)
    maps = as_format(random_q(rng, n, H, W), ld.F32)
    poses = generic_poses(rng, n)
    p = localmap.localmap_params(ld.F32, min_hits=1, min_floor=1)
    runs = []
    for _ in range(2):
        with localmap.LocalMap(p, max_batch=n) as m:
            a = gpu_update(m, sp, poses, maps)
            m.recenter(0.7, -0.4)
            b = gpu_update(m, sp, poses[::-1], maps[::-1].copy())
            runs.append(a + b + m.read())
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))

"""Every kernel behind a disparity map under every rig of tests/rigs.py — the shipped rig is only one row of that table.  The mono8 tail
(u8 map, valid-disparity table, both scan flavours, point cloud) against tests/scan_def.py, which tests/test_scan_def.py pins to the
oracle; the costmap, the sub-pixel tail and the local map against their own definitions with their own comparisons; the device-against-
device anchors; the fused SGM tail against the separate calls; the ground estimator on a floor rendered for the rig.  Each test asserts
that the rig reaches the path its row of the table names."""
import functools
import math

import numpy as np
import pytest

import costmap_check as cc
import ground_def as gd
import localmap_check as lc
import localmap_def as ld
import rigs
import scan_def as sdef
import subpix_check as sc
import subpix_def as sd

pytestmark = pytest.mark.gpu

SCAN_TOL, MARGIN = sc.SCAN_TOL, sc.MARGIN          # the project's scan tolerance and bin-edge margin: one definition (tests/subpix_check.py)
SHAPES = [(200, 37), (321, 49), (257, 17)]       # under one 256-column block and no multiple of the 16-row strip; two blocks, the second nearly
#                                                   empty; one column in the second block and one row in the second strip
NODE_SHAPES = SHAPES + [(1, 33), (513, 1)]
N = 3
FORMATS = sc.FORMATS
GRID = dict(cells_x=48, cells_y=40, resolution=0.13, origin_x=-3.1, origin_y=-2.6, min_hits=2)     # around the robot: the rigs look everywhere


@functools.lru_cache(maxsize=None)
def node_inputs(W, H):
    """(float maps, their u8 form by the definition) [N][H][W]: shared by the tests, never written."""
    D = rigs.float_maps(np.random.default_rng(1000 + 7 * W + H), N, H, W)
    u8 = sdef.to_u8(D)
    D.setflags(write=False); u8.setflags(write=False)
    return D, u8


@functools.lru_cache(maxsize=None)
def q_inputs(W, H):
    q = sc.random_q(np.random.default_rng(2000 + 7 * W + H), N, H, W)
    q[:, ::5, ::3] = 112                                               # w = 0 under flipped_baseline_w0, often enough for the smallest shape
    q.setflags(write=False)
    return q


def rig(name, W, H):
    from jackal_navigation_amd import node
    return rigs.apply(name, node.scan_params(W, H), W, H)


@functools.lru_cache(maxsize=None)
def table(name, W, H):
    lut = sdef.valid_lut(rig(name, W, H), W, H)
    lut.setflags(write=False)
    return lut


@functools.lru_cache(maxsize=None)
def reached(name, which):
    """The rig does what its row says, on the inputs the tests use at the first shape."""
    W, H = SHAPES[0]
    sp = rig(name, W, H)
    if which == "u8":
        f = rigs.facts(sp, node_inputs(W, H)[1], table(name, W, H))
    else:
        q, valid = sd.to_q(q_inputs(W, H), sd.I16_SUB)
        f = rigs.facts(sp, q / 16.0, table(name, W, H), valid)
    return bool(rigs.REACHES[name](f)), {k: v for k, v in f.items() if k != "bins_hit"}


def assert_reaches(name, which="u8"):
    ok, f = reached(name, which)
    assert ok, (name, which, f)


def scan_outputs(n):
    def make(sp):
        from jackal_navigation_amd.device import DeviceArray
        return DeviceArray.from_numpy(np.full((n, sp.bins), 77.0)), DeviceArray.from_numpy(np.full((n, 4), 77.0))
    return make


def compare_scan(sp, bins, meta, want, what):
    """One frame against the definition's (bins, meta, edge) by the margin rule -> 1 if the bins were left out."""
    wb, wm, edge = want
    assert np.allclose(meta, wm, rtol=0, atol=SCAN_TOL), (what, meta.tolist(), wm.tolist())
    if edge <= MARGIN:
        return 1
    assert np.array_equal(bins < sdef.EMPTY - 1, wb < sdef.EMPTY - 1), (what, np.flatnonzero((bins < sdef.EMPTY - 1) != (wb < sdef.EMPTY - 1))[:8].tolist())
    assert np.allclose(bins, wb, rtol=0, atol=SCAN_TOL), what
    return 0


@pytest.mark.parametrize("name", rigs.NAMES)
def test_valid_disparity_table(jn, same, name):
    from jackal_navigation_amd import node
    for W, H in NODE_SHAPES:
        got = node.build_valid_disp_lut(rig(name, W, H), W, H).numpy()
        want = table(name, W, H)
        assert same(got, want), (name, W, H, int((got != want).sum()), np.argwhere(got[..., 0] != want[..., 0])[:4].tolist())
    assert_reaches(name)
    if name == "gp_steep":
        assert (table(name, *SHAPES[0])[-8:, :, 0] == 0).all()                 # the 256 -> 0 wrap, a whole row at a time


@pytest.mark.parametrize("name", rigs.NAMES)
def test_scan_both_flavours_both_routes(jn, same, name):
    from jackal_navigation_amd import node
    from jackal_navigation_amd.device import DeviceArray
    frames = left_out = 0
    for W, H in NODE_SHAPES:
        sp = rig(name, W, H)
        D, u8 = node_inputs(W, H)
        lut_np = table(name, W, H)
        dLut, dD, dU = DeviceArray.from_numpy(lut_np), DeviceArray.from_numpy(D), DeviceArray.from_numpy(u8)
        make = scan_outputs(N)
        # the float route: the u8 map it writes, then the LUT flavour; the cloud flavour from that map
        dOut = DeviceArray.from_numpy(np.full((N, H, W), 0xAB, np.uint8))
        fb, fm = make(sp)
        node.disparity_scan(sp, N, dD.ptr, dLut.ptr, W, H, dOut.ptr, fb.ptr, fm.ptr)
        assert same(dOut.numpy(), u8), (name, W, H)
        fcb, fcm = make(sp)
        node.obstacle_scan_cloud(sp, N, dOut.ptr, W, H, fcb.ptr, fcm.ptr)
        # the u8 route
        ub, um = make(sp)
        node.obstacle_scan(sp, N, dU.ptr, dLut.ptr, W, H, ub.ptr, um.ptr)
        ucb, ucm = make(sp)
        node.obstacle_scan_cloud(sp, N, dU.ptr, W, H, ucb.ptr, ucm.ptr)
        lutf = [a.numpy() for a in (fb, fm)]; cloudf = [a.numpy() for a in (fcb, fcm)]
        assert same(ub.numpy(), lutf[0]) and same(um.numpy(), lutf[1]), (name, W, H, "lut: float route != u8 route")
        assert same(ucb.numpy(), cloudf[0]) and same(ucm.numpy(), cloudf[1]), (name, W, H, "cloud: float route != u8 route")
        for f in range(N):
            left_out += compare_scan(sp, lutf[0][f], lutf[1][f], sdef.scan(sp, u8[f], lut_np), (name, W, H, f, "lut"))
            left_out += compare_scan(sp, cloudf[0][f], cloudf[1][f], sdef.scan_cloud(sp, u8[f]), (name, W, H, f, "cloud"))
            frames += 2
        # frame 1 alone: the same bits, so nothing leaks between frames through the LDS bins or the global extrema
        one = scan_outputs(1)
        d1 = DeviceArray.from_numpy(D[1:2]); u1 = DeviceArray.from_numpy(u8[1:2]); o1 = DeviceArray.from_numpy(np.full((1, H, W), 0xAB, np.uint8))
        b, m = one(sp); node.disparity_scan(sp, 1, d1.ptr, dLut.ptr, W, H, o1.ptr, b.ptr, m.ptr)
        assert same(b.numpy()[0], lutf[0][1]) and same(m.numpy()[0], lutf[1][1]) and same(o1.numpy()[0], u8[1]), (name, W, H)
        b, m = one(sp); node.obstacle_scan(sp, 1, u1.ptr, dLut.ptr, W, H, b.ptr, m.ptr)
        assert same(b.numpy()[0], lutf[0][1]) and same(m.numpy()[0], lutf[1][1]), (name, W, H)
        b, m = one(sp); node.obstacle_scan_cloud(sp, 1, u1.ptr, W, H, b.ptr, m.ptr)
        assert same(b.numpy()[0], cloudf[0][1]) and same(m.numpy()[0], cloudf[1][1]), (name, W, H)
        if (W, H) == SHAPES[0] and name != "gp_steep":                          # (under gp_steep every point is ground: the cloud flavour sees nothing)
            assert (cloudf[0] < sdef.EMPTY - 1).any() and (lutf[0] < sdef.EMPTY - 1).any()
    assert 20 * left_out <= frames, (left_out, frames)
    assert_reaches(name)


@pytest.mark.parametrize("name", rigs.NAMES)
def test_point_cloud_is_the_definitions_bits(jn, same, name):
    from jackal_navigation_amd import node
    from jackal_navigation_amd.device import DeviceArray
    zeros = 0
    for W, H in NODE_SHAPES:
        sp = rig(name, W, H)
        u8 = node_inputs(W, H)[1]
        for f in range(N):
            dU = DeviceArray.from_numpy(u8[f])
            got = node.point_cloud(sp, dU.ptr, W, H)
            want = sdef.cloud(sp, u8[f])
            assert got.shape == want.shape == (int((u8[f] >= 2).sum()), 3), (name, W, H, f)
            assert same(got, want), (name, W, H, f, int((got.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()))
            zeros += int((~sdef.cloud_w_nonzero(sp, u8[f])).sum())
            dU.free()
    assert (zeros > 0) == (name == "flipped_baseline_w0")                      # the w = 0 rows: (0, 0, 0)
    assert_reaches(name)


@pytest.mark.parametrize("from_cloud", [0, 1])
@pytest.mark.parametrize("name", rigs.NAMES)
def test_costmap(jn, same, name, from_cloud):
    from jackal_navigation_amd import costmap
    from jackal_navigation_amd.device import DeviceArray
    cp = costmap.costmap_params(from_cloud=from_cloud, **GRID)
    total = 0
    for W, H in SHAPES:
        sp = rig(name, W, H)
        u8 = np.array(node_inputs(W, H)[1])
        lut_np = table(name, W, H)
        lut = DeviceArray.from_numpy(lut_np)
        hits, grid, bins = cc.run_costmap(sp, cp, u8, lut)
        cc.check_against_definition(sp, cp, u8, lut_np, hits, grid, bins, (name, W, H, from_cloud))
        h1, g1, b1 = cc.run_costmap(sp, cp, u8[1:2], lut)
        assert same(h1[0], hits[1]) and same(g1[0], grid[1]) and same(b1[0], bins[1]), (name, W, H)
        total += int(hits.sum())
    assert total > 0 or (name == "gp_steep" and from_cloud)                    # (every point is ground there)
    assert_reaches(name)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", rigs.NAMES)
def test_subpixel_tail(jn, same, name, fmt):
    from jackal_navigation_amd import costmap, subpix
    cp = costmap.costmap_params(**GRID)
    fp = subpix.subpix_params(fmt)
    frames = left_out = total = 0
    for W, H in SHAPES:
        sp = rig(name, W, H)
        maps = sc.as_format(q_inputs(W, H), fmt, np.random.default_rng(W + fmt))
        out = sc.run(sp, cp, fp, maps)
        left_out += sc.check_against_definition(sp, cp, fp, maps, out, (name, fmt, W, H))
        frames += N
        one = sc.run(sp, cp, fp, maps[1:2], want_cloud=False)
        for k in ("scan_bins", "scan_meta", "hits", "grid"):
            assert same(one[k][0], out[k][1]), (name, fmt, W, H, k)
        total += int(out["hits"].sum())
    assert 20 * left_out <= frames, (left_out, frames)
    assert total > 0 or name == "gp_steep"
    assert_reaches(name, "q")


@pytest.mark.parametrize("name", rigs.NAMES)
def test_local_map(jn, name):
    """One update under the zero pose, one under other poses; a format per shape."""
    from jackal_navigation_amd import localmap
    total = 0
    for (W, H), fmt in zip(SHAPES, FORMATS):
        sp = rig(name, W, H)
        maps = lc.as_format(q_inputs(W, H), fmt)
        p = localmap.localmap_params(fmt, cells_x=64, cells_y=56, resolution=0.11, min_hits=2, min_floor=2)
        ref = ld.Map(p)
        rng = np.random.default_rng(W)
        with localmap.LocalMap(p, max_batch=N) as m:
            o, f = lc.step(m, ref, sp, [(0.0, 0.0, 0.0)] * N, maps, (name, W, H, "zero pose"))
            total += int(o.sum()) + int(f.sum())
            o, f = lc.step(m, ref, sp, [(0.4, -0.3, 2.5)] + lc.generic_poses(rng, N - 1), maps, (name, W, H, "poses"))
            total += int(o.sum()) + int(f.sum())
    assert total > 0
    assert_reaches(name, "q")


@pytest.mark.parametrize("name", rigs.NAMES)
def test_anchors_device_against_device(jn, same, name):
    """On integer maps jn_subpix_scan is jn_obstacle_scan_cloud and the sub-pixel cloud is jn_point_cloud; under the zero pose the local
    map's obstacle counts are jn_subpix_costmap's hits.  Bit for bit, under every rig."""
    from jackal_navigation_amd import costmap, localmap, node, subpix
    from jackal_navigation_amd.device import DeviceArray
    for W, H in SHAPES:
        sp = rig(name, W, H)
        u8 = np.array(node_inputs(W, H)[1])
        dU = DeviceArray.from_numpy(u8)
        bins, meta = scan_outputs(N)(sp)
        node.obstacle_scan_cloud(sp, N, dU.ptr, W, H, bins.ptr, meta.ptr)
        cloud = node.point_cloud(sp, dU.ptr, W, H)
        for fmt in FORMATS:
            maps = {sd.F32: u8.astype(np.float32), sd.I16: u8.astype(np.int16), sd.I16_SUB: u8.astype(np.int16) * 16}[fmt]
            out = sc.run(sp, None, subpix.subpix_params(fmt), maps)
            assert same(out["scan_bins"], bins.numpy()) and same(out["scan_meta"], meta.numpy()), (name, W, H, fmt)
            assert same(out["cloud"], cloud), (name, W, H, fmt)
            p = localmap.localmap_params(fmt, cells_x=96, cells_y=80, resolution=0.07)
            qmaps = lc.as_format(q_inputs(W, H), fmt)
            with localmap.LocalMap(p, max_batch=N) as m:
                w = m.window()
                o, f = lc.gpu_update(m, sp, [(0.0, 0.0, 0.0)] * N, qmaps)
            cp = costmap.costmap_params(origin_x=w.origin[0], origin_y=w.origin[1], resolution=p.resolution, cells_x=96, cells_y=80)
            got = sc.run(sp, cp, subpix.subpix_params(fmt), qmaps, want_cloud=False)
            assert same(o, got["hits"]), (name, W, H, fmt, int((o != got["hits"]).sum()))
            assert o.sum() > 0 or name == "gp_steep"
    assert_reaches(name)


@pytest.mark.parametrize("lr", [-1, 1])
@pytest.mark.parametrize("subpixel", [0, 1])
@pytest.mark.parametrize("name", ["pitched_yawed_rolled", "rear_fov360"])
def test_fused_sgm_tail_equals_the_separate_calls(jn, same, name, subpixel, lr):
    """k_scan<false, true>: an SGM handle's scan route against jn_sgm_process_batch -> jn_sgm_disparity_to_u8 -> jn_obstacle_scan.
    D = 64: the smallest disparity range jn_sgm_create accepts (64, 128 or 256; 32 is JN_ERR_UNSUPPORTED)."""
    from jackal_navigation_amd import node
    from jackal_navigation_amd.device import DeviceArray
    W, H, B = 270, 49, 2
    sp = rig(name, W, H)
    dLut = DeviceArray.from_numpy(table(name, W, H))
    pairs = [node.synth_pair(W, H, 20, 700 + t) for t in range(B)]
    dL = DeviceArray.from_numpy(np.stack([a for a, _ in pairs])); dR = DeviceArray.from_numpy(np.stack([b for _, b in pairs]))
    dd = DeviceArray.from_numpy(np.full((B, H, W), 0x5A5A, np.int16)); u8 = DeviceArray.from_numpy(np.full((B, H, W), 0xAB, np.uint8))
    bins, meta = scan_outputs(B)(sp)
    dd2 = DeviceArray.from_numpy(np.full((B, H, W), 0x5A5A, np.int16)); u82 = DeviceArray.from_numpy(np.full((B, H, W), 0xAB, np.uint8))
    bins2, meta2 = scan_outputs(B)(sp)
    with jn.Sgm(jn.Sgm.parameters(num_disparities=64, subpixel=subpixel, lr_max_diff=lr), W, H, max_batch=B) as m:
        m.submit_scan(0, B, dL.ptr, dR.ptr, W, H * W, dd.ptr, sp, dLut.ptr, u8.ptr, bins.ptr, meta.ptr)
        m.wait(0)
        m.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd2.ptr)
        m.to_u8(dd2.ptr, u82.ptr, B * H * W)
    node.obstacle_scan(sp, B, u82.ptr, dLut.ptr, W, H, bins2.ptr, meta2.ptr)
    assert same(dd.numpy(), dd2.numpy()) and same(u8.numpy(), u82.numpy())
    assert same(bins.numpy(), bins2.numpy()) and same(meta.numpy(), meta2.numpy())
    maps = u8.numpy()
    assert (maps >= 3).mean() > 0.3 and (bins.numpy() < sdef.EMPTY - 1).sum() >= 4
    if subpixel:
        v = dd.numpy()
        assert (v[v > 0] % 16 != 0).any()
    if lr >= 0:
        assert (dd.numpy() < 0).any()                                            # the check refused something
    f = rigs.facts(sp, maps, table(name, W, H), maps >= 3)
    assert f["strip_bin_changes"] > 0 if name == "pitched_yawed_rolled" else f["x_negative"] > 0, f     # on the matcher's own map


@pytest.mark.parametrize("name", rigs.SEES_A_FLOOR)
def test_ground_estimator_gives_back_the_rig(jn, name):
    """A floor rendered for the rig (tests/ground_def.py floor_disparity) plus noise and a wall: the device's refit sums are the definition's,
    and the plane gives back the rig's XR / XT from a prior 3.6 degrees and 5 cm off, to what tests/test_gpu_ground.py allows."""
    from jackal_navigation_amd import ground
    from jackal_navigation_amd.device import DeviceArray
    W, H, n, noise = 480, 270, 2, 0.3
    sp = rig(name, W, H)
    XRt, XTt = np.array(sp.XR).reshape(3, 3), np.array(sp.XT)
    rng = np.random.default_rng(21)
    d = gd.floor_disparity(sp, XRt, XTt, W, H)
    maps = np.empty((n, H, W), np.float32)
    for f in range(n):
        m = d + rng.uniform(-noise, noise, (H, W))
        m[d < 1.0] = -10.0                                                       # at and above the horizon
        m[H // 2:H // 2 + 15] = 30.0 + rng.uniform(-noise, noise, (15, W))       # a wall across the top of the region
        maps[f] = m
    gp = ground.ground_params(W, H, hypotheses=64)
    dD = DeviceArray.from_numpy(maps)
    planes, scores, hyps = ground.estimate(sp, gp, n, dD.ptr, gd.F32, W, H, want_scores=True)
    up = XRt[2] / np.linalg.norm(XRt[2])
    for f in range(n):
        e = gd.frame(maps[f], gd.F32, f, gp, sp)
        p = planes[f]
        assert np.array_equal(hyps[f], e["hyps"]) and np.array_equal(scores[f], e["scores"]), (name, f)
        assert p.best == e["best"] and list(p.sums) == e["sums"] and p.valid == e["valid"] and p.status == e["status"] == 0, (name, f, list(p.sums), e["sums"])
        assert p.inliers > 0.6 * p.valid and p.rms < 0.25, (name, f, p.inliers, p.valid, p.rms)
        assert math.degrees(math.acos(min(1.0, float(np.dot(list(p.n_cam), up))))) < 0.05 and abs(p.height_m - XTt[2]) < 0.002, (name, f, list(p.n_cam), p.height_m)
        assert np.allclose(list(p.n_cam), e["n_cam"], rtol=0, atol=1e-12) and p.height_m == pytest.approx(e["height_m"], rel=1e-9, abs=1e-12)
    prior = rig(name, W, H)
    prior.XR[:] = (gd.rot_xyz(2.0, -3.0) @ XRt).reshape(-1).tolist()
    prior.XT[:] = [float(XTt[0]), float(XTt[1]), float(XTt[2]) + 0.05]
    XR, XT, tilt = ground.extrinsics(planes, prior)
    assert 3.0 < tilt < 4.2
    assert math.degrees(math.acos(min(1.0, float(XR[2] @ up)))) < 0.05 and abs(XT[2] - XTt[2]) < 0.002, (name, XR.tolist(), XT.tolist())
    assert np.allclose(XR @ XR.T, np.eye(3), atol=1e-7)


def test_to_u8_on_the_values_that_decide_it(jn, same):
    from jackal_navigation_amd import node
    from jackal_navigation_amd.device import DeviceArray
    v = rigs.decisive_floats()
    dD = DeviceArray.from_numpy(v); out = DeviceArray.from_numpy(np.full(v.shape, 0xAB, np.uint8))
    node.disparity_to_u8(dD.ptr, out.ptr, v.size)
    assert same(out.numpy(), sdef.to_u8(v)), v[out.numpy() != sdef.to_u8(v)][:8].tolist()
    # the same values through the scan's own conversion (k_scan converts in its first phase, not through k_to_u8)
    sp = rig("default", v.size, 1)
    dLut = DeviceArray.from_numpy(table("default", v.size, 1))
    bins, meta = scan_outputs(1)(sp)
    out2 = DeviceArray.from_numpy(np.full((1, 1, v.size), 0xAB, np.uint8))
    node.disparity_scan(sp, 1, dD.ptr, dLut.ptr, v.size, 1, out2.ptr, bins.ptr, meta.ptr)
    assert same(out2.numpy().reshape(-1), sdef.to_u8(v))
    # non-finite values: ELAS never emits them and the reference does not define them; include/jn_stereo.h states these answers
    nf = DeviceArray.from_numpy(np.array([np.nan, np.inf, -np.inf], np.float32)); o3 = DeviceArray.from_numpy(np.full(3, 0xAB, np.uint8))
    node.disparity_to_u8(nf.ptr, o3.ptr, 3)
    assert o3.numpy()[0] == 0                                                    # NaN
    assert o3.numpy()[1] == 255                                                  # +inf
    assert o3.numpy()[2] == 0                                                    # -inf
    sp3 = rig("default", 3, 1)
    l3 = DeviceArray.from_numpy(table("default", 3, 1)); b3, m3 = scan_outputs(1)(sp3); o4 = DeviceArray.from_numpy(np.full((1, 1, 3), 0xAB, np.uint8))
    node.disparity_scan(sp3, 1, nf.ptr, l3.ptr, 3, 1, o4.ptr, b3.ptr, m3.ptr)
    assert o4.numpy().reshape(-1).tolist() == [0, 255, 0]                        # k_scan's conversion says the same

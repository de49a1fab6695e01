"""The ground-plane estimator (include/jn_ground.h) on the GPU against its definition (tests/ground_def.py): hypotheses, scores, winner
and refit sums bit-identical in the three formats; round-half-even of the float format; the geometry (a rendered floor of the default rig
gives back its normal and height, and the scan stops seeing the floor); real matcher output; walls refused."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ground_def as gd
from scenes import make_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {gd.F32: np.float32, gd.I16: np.int16, gd.I16_SUB: np.int16}


def random_maps(rng, n, H, W, fmt):
    """A floor (a plane that rises down the image) + noise + an obstacle box + holes of invalid pixels, in the format's units."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W), DTYPES[fmt])
    for f in range(n):
        beta, alpha = rng.uniform(0.1, 0.5), rng.uniform(-0.05, 0.05)
        d = beta * (yy - 0.3 * H) + alpha * xx + rng.uniform(1, 4) + rng.uniform(-0.4, 0.4, (H, W))
        x0, x1 = sorted(rng.integers(0, W + 1, 2)); y0, y1 = sorted(rng.integers(0, H + 1, 2))
        d[y0:y1, x0:x1] = rng.uniform(5, 40)                            # a box facing the camera
        invalid = rng.random((H, W)) < 0.15
        for _ in range(4):
            hx, hy = rng.integers(0, W), rng.integers(0, H)
            invalid[hy:hy + max(1, H // 6), hx:hx + max(1, W // 5)] = True
        if fmt == gd.F32:
            m = d.astype(np.float32)
            m[invalid] = -10.0                                           # ELAS's invalid value
            m[rng.random((H, W)) < 0.01] = np.nan
            m[rng.random((H, W)) < 0.01] = np.inf
            m[rng.random((H, W)) < 0.01] = 1e30
        elif fmt == gd.I16:
            m = np.rint(d).astype(np.int16)
            m[invalid] = -1
            m[rng.random((H, W)) < 0.01] = 32767
        else:
            m = np.rint(16 * d).astype(np.int16)
            m[invalid] = -16
            m[rng.random((H, W)) < 0.01] = -32768
        out[f] = m
    return out


def run(sp, gp, maps, fmt, offset_elements=0):
    """maps [n][H][W] (numpy) -> (planes, scores, hyps).  offset_elements: the maps start that many elements into the device allocation
    (an address the wide loads cannot use)."""
    from jackal_navigation_amd import ground
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = maps.shape
    flat = np.concatenate([np.zeros(offset_elements, maps.dtype), maps.reshape(-1)])
    d = DeviceArray.from_numpy(flat)
    try:
        return ground.estimate(sp, gp, n, d.ptr + offset_elements * maps.dtype.itemsize, fmt, W, H, want_scores=True)
    finally:
        d.free()


def check(sp, gp, maps, fmt, what, offset_elements=0):
    planes, scores, hyps = run(sp, gp, maps, fmt, offset_elements)
    for f in range(maps.shape[0]):
        e = gd.frame(maps[f], fmt, f, gp, sp)
        assert np.array_equal(hyps[f], e["hyps"]), (what, f, "hyps", int((hyps[f] != e["hyps"]).any(axis=1).sum()))
        bad = np.nonzero(scores[f] != e["scores"])[0]
        assert bad.size == 0, (what, f, "scores", bad[:5].tolist(), scores[f][bad[:5]].tolist(), e["scores"][bad[:5]].tolist())
        p = planes[f]
        assert p.best == e["best"] and p.inliers == e["sums"][0] == int(e["scores"][e["best"]]), (what, f, p.best, e["best"])
        assert list(p.sums) == e["sums"] and p.valid == e["valid"], (what, f, list(p.sums), e["sums"])
        assert p.status == e["status"], (what, f)
        for k in ("a", "b", "c", "rms", "height_m"):
            assert getattr(p, k) == pytest.approx(e[k], rel=1e-9, abs=1e-12), (what, f, k)
        assert np.allclose(list(p.n_cam), e["n_cam"], rtol=0, atol=1e-12), (what, f)
    return planes


# W, H, (x0, y0, x1, y1) or None for the default region, K, n, dict of other fields
CASES = [
    (8, 8, (0, 0, 8, 8), 64, 2, {}),
    (97, 61, (5, 30, 90, 61), 64, 3, {}),                     # width 85; rows and the array end off the four-element grid
    (97, 61, (96, 0, 97, 61), 64, 1, {}),                     # one column: every hypothesis degenerate
    (333, 100, (7, 50, 331, 51), 64, 1, {}),                  # one row high
    (320, 180, None, 256, 2, {}),
    (320, 180, None, 256, 1, {"tol_q": 0}),
    (320, 180, (1, 90, 258, 180), 128, 1, {"seed": 12345, "tol_q": 3}),       # 257 wide: two runs, the second one pixel
    (640, 360, None, 1024, 1, {"min_disp": 3}),
    (64, 48, None, 64, 33, {"seed": 7}),
    (1920, 1080, None, 64, 1, {}),
]


@pytest.mark.parametrize("fmt", [gd.F32, gd.I16, gd.I16_SUB])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_maps_equal_the_definition(jn, case, fmt):
    from jackal_navigation_amd import ground, node
    W, H, roi, K, n, kw = CASES[case]
    if (W, K) in ((1920, 64), (640, 1024)) and fmt == gd.I16:
        pytest.skip("the big cases run in the float and the sub-pixel format")
    rng = np.random.default_rng(1000 * case + fmt)
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H, hypotheses=K, min_inliers=20, **kw)
    if roi:
        gp.roi_x0, gp.roi_y0, gp.roi_x1, gp.roi_y1 = roi
    maps = random_maps(rng, n, H, W, fmt)
    planes = check(sp, gp, maps, fmt, (case, fmt))
    if case in (4, 7, 9):
        assert all(p.status == 0 and p.inliers > 0.3 * p.valid for p in planes)      # the floor is found
    if case in (2, 3):
        assert all(p.status == 1 and p.inliers == 0 for p in planes)


@pytest.mark.parametrize("fmt", [gd.F32, gd.I16, gd.I16_SUB])
def test_maps_at_an_address_the_wide_loads_cannot_use(jn, fmt):
    from jackal_navigation_amd import ground, node
    W, H = 131, 77
    rng = np.random.default_rng(77 + fmt)
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H, hypotheses=64, min_inliers=20)
    maps = random_maps(rng, 2, H, W, fmt)
    for off in (1, 2, 3):
        check(sp, gp, maps, fmt, ("offset", off, fmt), offset_elements=off)


@pytest.mark.parametrize("fmt", [gd.F32, gd.I16, gd.I16_SUB])
def test_an_all_invalid_map_has_no_floor(jn, fmt):
    from jackal_navigation_amd import ground, node, _lib
    W, H = 160, 120
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H, hypotheses=64)
    maps = np.full((2, H, W), {gd.F32: -10.0, gd.I16: -1, gd.I16_SUB: -16}[fmt], DTYPES[fmt])
    planes, scores, hyps = run(sp, gp, maps, fmt)
    assert not scores.any() and not hyps.any()
    for p in planes:
        assert p.status == _lib.JN_ERR_FEW_SUPPORT and p.best == 0 and p.inliers == 0 and p.valid == 0 and list(p.sums) == [0] * 10
        assert p.height_m == 0 and p.a == 0
    with pytest.raises(_lib.JnError) as e:
        ground.extrinsics(planes, sp)
    assert e.value.status == _lib.JN_ERR_FEW_SUPPORT


def test_float_maps_round_half_to_even(jn):
    """Maps made of k / 32: the odd k are exact halves in 1/16 pixel."""
    from jackal_navigation_amd import ground, node
    W, H = 128, 64
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H, hypotheses=64, tol_q=0, min_inliers=10, beta_min=0.001)
    yy, xx = np.mgrid[0:H, 0:W]
    k = 2 * (8 * yy + xx) + 1 + 64                                        # odd everywhere: every pixel is a tie
    maps = (k / 32.0).astype(np.float32)[None]
    assert (maps * 32 == k).all()
    q, valid = gd.to_q(maps[0], gd.F32, gp.min_disp)
    assert valid.all() and (q % 2 == 0).all() and (np.abs(q - k / 2.0) == 0.5).all()
    planes = check(sp, gp, maps, gd.F32, "ties")
    # the rounded map is not a plane (q alternates between k/2 - 1/2 and k/2 + 1/2), so with tol_q = 0 only part of the region is on the winner
    assert 0 < planes[0].inliers < planes[0].valid
    # rounding away from zero or towards it would give different sums
    for other in (np.floor(k / 2.0 + 0.5), np.floor(k / 2.0)):
        assert int(other[H // 2:].sum()) != int(q[H // 2:].sum())


def _floor_maps(sp, W, H, rng, n, noise=0.3, wall_rows=40):
    XR, XT = np.array(sp.XR).reshape(3, 3), np.array(sp.XT)
    d = gd.floor_disparity(sp, XR, XT, W, H)
    maps = np.empty((n, H, W), np.float32)
    for f in range(n):
        m = d + rng.uniform(-noise, noise, (H, W))
        m[d < 1.0] = -10.0                                               # at and above the horizon
        m[H // 2:H // 2 + wall_rows] = 30.0 + rng.uniform(-noise, noise, (wall_rows, W))   # a wall across the top of the region
        maps[f] = m
    return maps, d


def test_a_rendered_floor_gives_back_the_rig(jn):
    from jackal_navigation_amd import ground, node
    from jackal_navigation_amd.device import DeviceArray
    W, H, n = 1280, 720, 4
    rng = np.random.default_rng(11)
    sp = node.scan_params(W, H)                                           # the truth: the default rig
    XRt, XTt = np.array(sp.XR).reshape(3, 3), np.array(sp.XT)
    maps, d_true = _floor_maps(sp, W, H, rng, n)
    gp = ground.ground_params(W, H)
    planes, scores, hyps = run(sp, gp, maps, gd.F32)
    up = XRt[2] / np.linalg.norm(XRt[2])
    for p in planes:
        assert p.status == 0 and p.inliers > 0.6 * p.valid and p.rms < 0.25
        assert math.degrees(math.acos(min(1.0, float(np.dot(list(p.n_cam), up))))) < 0.05 and abs(p.height_m - 0.28) < 0.002
    # a prior pitched 3 degrees (nose down: the floor ahead seems to rise), rolled 2 degrees and 5 cm too high
    prior = node.scan_params(W, H)
    prior.XR[:] = (gd.rot_xyz(2.0, -3.0) @ XRt).reshape(-1).tolist()
    prior.XT[:] = [0.0, 0.0, 0.33]
    XR, XT, tilt = ground.extrinsics(planes, prior)
    assert 3.0 < tilt < 4.2
    assert math.degrees(math.acos(min(1.0, float(XR[2] @ up)))) < 0.05 and abs(XT[2] - 0.28) < 0.002
    assert np.allclose(XR @ XR.T, np.eye(3), atol=1e-7)                   # as orthonormal as the shipped matrix it started from
    # the same from the nominal prior (what a rig without XR / XT starts from)
    nominal = node.scan_params(W, H)
    XR0, XT0 = ground.nominal_prior()
    nominal.XR[:] = XR0.reshape(-1).tolist(); nominal.XT[:] = XT0.tolist()
    XRn, XTn, tiltn = ground.extrinsics(planes, nominal)
    assert abs(tiltn - 15.5) < 0.2 and math.degrees(math.acos(min(1.0, float(XRn[2] @ up)))) < 0.05 and abs(XTn[2] - 0.28) < 0.002
    # the scan: the clean floor (as the u8 map the node publishes), binned with the wrong prior and with the estimate
    clean = np.where(d_true >= 2.0, np.rint(d_true), 0).astype(np.uint8)[None]
    dD = DeviceArray.from_numpy(clean)
    hit = {}
    est = node.scan_params(W, H)
    est.XR[:] = XR.reshape(-1).tolist(); est.XT[:] = XT.tolist()
    for name, s in (("prior", prior), ("estimate", est)):
        bins = DeviceArray((1, s.bins), np.float64); meta = DeviceArray((1, 4), np.float64)
        node.obstacle_scan_cloud(s, 1, dD.ptr, W, H, bins.ptr, meta.ptr)
        hit["cloud " + name] = int((bins.numpy() < 1e9 - 1).sum())
        lut = node.build_valid_disp_lut(s, W, H)
        node.obstacle_scan(s, 1, dD.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
        hit["lut " + name] = int((bins.numpy() < 1e9 - 1).sum())
    assert hit["cloud prior"] > 0 and hit["cloud estimate"] == 0, hit      # the floor was an obstacle; it no longer is
    assert hit["lut estimate"] <= hit["lut prior"] and hit["lut estimate"] == 0, hit


@pytest.mark.parametrize("matcher", ["elas", "sgm_sub"])
def test_real_matcher_output(jn, matcher):
    """The slanted scene (disparity grows along x and y) through a matcher: the fitted plane agrees with the least-squares plane of the
    scene's true disparity to 0.25 px rms over the region."""
    from jackal_navigation_amd import ground, node
    from matcher_run import run as run_matcher
    W, H, dmax = 320, 180, 64
    L, R = make_scene("slanted", W, H, dmax, 3)
    yy, xx = np.mgrid[0:H, 0:W]
    truth = (2 + xx * (0.35 * dmax) / W + yy * (0.3 * dmax) / H).astype(np.int64).astype(np.float64)
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H, tol_q=16)
    gp.roi_x0 = dmax                                                       # left of it the right image has no counterpart
    if matcher == "elas":
        D1 = np.zeros((H, W), np.float32); D2 = np.zeros((H, W), np.float32)
        with jn.Elas(jn.Elas.parameters(jn.Elas.ROBOTICS, disp_max=dmax - 1), W, H) as e:
            assert e.process(L, R, D1, D2, (W, H, W)) == 0
        maps, fmt = D1[None], gd.F32
    else:
        out, _, _ = run_matcher(jn, jn.Sgm, jn.Sgm.parameters(num_disparities=dmax, subpixel=1), L[None], R[None])
        maps, fmt = out, gd.I16_SUB
    planes = check(sp, gp, np.ascontiguousarray(maps), fmt, matcher)
    p = planes[0]
    assert p.status == 0 and p.inliers > 0.5 * p.valid, (p.inliers, p.valid)
    ys, xs = yy[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1].reshape(-1), xx[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1].reshape(-1)
    A = np.stack([xs, ys, np.ones_like(xs)], 1).astype(np.float64)
    coef = np.linalg.lstsq(A, truth[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1].reshape(-1), rcond=None)[0]
    diff = A @ (np.array([p.a, p.b, p.c]) - coef)
    assert math.sqrt(float((diff ** 2).mean())) < 0.25, (matcher, (p.a, p.b, p.c), coef.tolist())


def test_a_wall_is_never_returned_as_a_floor(jn):
    from jackal_navigation_amd import ground, node, _lib
    W, H = 640, 360
    rng = np.random.default_rng(3)
    sp = node.scan_params(W, H)
    gp = ground.ground_params(W, H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    facing = (25.0 + rng.uniform(-0.3, 0.3, (H, W))).astype(np.float32)                         # constant disparity
    side = (5.0 + 0.12 * xx + rng.uniform(-0.3, 0.3, (H, W))).astype(np.float32)                # disparity grows along x only
    ceiling = (60.0 - 0.3 * yy + rng.uniform(-0.3, 0.3, (H, W))).astype(np.float32)             # disparity falls down the image
    for name, m in (("facing", facing), ("side", side), ("ceiling", ceiling)):
        planes, scores, hyps = run(sp, gp, m[None], gd.F32)
        p = planes[0]
        if p.status == _lib.JN_OK:                                         # whatever passed the gate must fail the tilt limit
            with pytest.raises(_lib.JnError) as e:
                ground.extrinsics(planes, sp)
            assert e.value.status == _lib.JN_ERR_INVALID, name
        else:
            assert p.status == _lib.JN_ERR_FEW_SUPPORT and p.height_m == 0, name
            with pytest.raises(_lib.JnError):
                ground.extrinsics(planes, sp)
    # with the gate wide open the side wall is fitted, and the tilt limit is what refuses it
    open_gate = ground.ground_params(W, H, beta_min=-64.0, alpha_max=64.0)
    planes, _, _ = run(sp, open_gate, side[None], gd.F32)
    assert planes[0].status == _lib.JN_OK and abs(planes[0].a - 0.12) < 0.01
    with pytest.raises(_lib.JnError) as e:
        ground.extrinsics(planes, sp)
    assert e.value.status == _lib.JN_ERR_INVALID


def render_floor_pair(sp, XR, XT, W, H, seed):
    """A rectified pair of the robot-frame plane z = 0: the right image is a band-limited texture, the left one samples it at x - d(x, y)
    (linear interpolation), d the floor's exact disparity; above the horizon d = 0.  -> (L, R, d)."""
    from scenes import _binomial_blur
    rng = np.random.default_rng(seed)
    t = _binomial_blur(rng.integers(0, 256, (H, W + 512)), 2).astype(np.float64)
    t = (t - t.min()) * 255.0 / (t.max() - t.min())
    d = np.maximum(gd.floor_disparity(sp, XR, XT, W, H), 0.0)
    yy, xx = np.mgrid[0:H, 0:W]
    pos = xx - d + 256.0
    i0 = np.floor(pos).astype(np.int64)
    w = pos - i0
    L = (1 - w) * t[yy, np.clip(i0, 0, W + 511)] + w * t[yy, np.clip(i0 + 1, 0, W + 511)]
    return np.rint(L).astype(np.uint8), np.rint(t[:, 256:256 + W]).astype(np.uint8), d


def test_ground_calibrate_tool_on_a_rendered_floor_pair(jn, tmp_path):
    """scripts/ground_calibrate.py end to end: the shipped rig's file with XR / XT reset to identity / zero (so the nominal prior is used)
    plus rendered floor pairs through ELAS -> a file whose XR / XT put the floor at z = 0."""
    import json
    import subprocess
    import sys
    from jackal_navigation_amd import node
    W, H = 640, 360
    c, XRt, XTt, present = jn.load_calibration(os.path.join(ROOT, "tests", "golden", "amrl_jackal_webcam_stereo.yml"))
    rig = str(tmp_path / "rig.yml"); out = str(tmp_path / "out.yml")
    jn.save_calibration(rig, c, np.eye(3), np.zeros(3))
    sp = node.scan_params(W, H)
    sp.Q[:] = list(node.stereo_rectify(c, W, H).Q)                        # the tool's Q: stereoRectify of the file at the working size
    lefts, rights = [], []
    for i in range(2):
        L, R, d = render_floor_pair(sp, XRt, XTt, W, H, 100 + i)
        lefts.append(str(tmp_path / ("l%d.npy" % i))); rights.append(str(tmp_path / ("r%d.npy" % i)))
        np.save(lefts[-1], L); np.save(rights[-1], R)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ground_calibrate.py"), rig, "--left", *lefts, "--right", *rights, "--rectified",
                        "--size", "%dx%d" % (W, H), "--write", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["prior"] == "nominal" and line["frames_ok"] == 2 and line["written"] == out
    c2, XR, XT, present = jn.load_calibration(out)
    assert present == 255 and bytes(c2.K1) == bytes(c.K1) and XR.reshape(-1).tolist() == line["XR"]
    up = XRt[2] / np.linalg.norm(XRt[2])
    angle = math.degrees(math.acos(min(1.0, float(XR[2] @ up))))
    # a real matcher's map, not a rendered disparity: ELAS's own error on a slanted, interpolated surface is what is left
    assert angle < 0.3 and abs(XT[2] - XTt[2]) < 0.01, (angle, XT[2], line["frames"])
    # the estimated floor is z = 0: the true floor's points, through the written XR / XT, lie within a centimetre of it out to 5 m
    Q = np.array(sp.Q).reshape(4, 4)
    ys, xs = np.mgrid[H // 2:H:7, 0:W:11]
    v = np.stack([xs, ys, d[ys, xs], np.ones_like(xs)], -1).reshape(-1, 4).astype(np.float64)
    v = v[v[:, 2] >= 2.0]
    pos = v @ Q.T
    cam = pos[:, :3] / pos[:, 3:4]
    rob = cam @ XR.T + XT
    near = rob[:, 0] < 5.0
    assert near.sum() > 100 and np.abs(rob[near, 2]).max() < 0.02, float(np.abs(rob[near, 2]).max())
    # --disparity with the exact map, --prior file on the file just written: the tilt left over is small
    np.save(str(tmp_path / "d.npy"), np.where(d >= 1.0, d, -10.0).astype(np.float32))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ground_calibrate.py"), out, "--disparity", str(tmp_path / "d.npy"),
                        "--size", "%dx%d" % (W, H)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line2 = json.loads(r.stdout.strip().splitlines()[-1])
    assert line2["prior"] == "file" and line2["tilt_from_prior_deg"] < 0.3 and abs(line2["height_m"] - XTt[2]) < 0.002
    XR2 = np.array(line2["XR"]).reshape(3, 3)
    assert math.degrees(math.acos(min(1.0, float(XR2[2] @ up)))) < 0.05

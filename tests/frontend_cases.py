"""The case tables of the camera front end's tests, shared by the CPU side (tests/test_rectify.py, tests/test_jpeg.py) and the GPU
side (tests/test_gpu_frontend.py) so that the two cannot drift apart.  TEST INFRASTRUCTURE: inputs only, no expected values."""
import numpy as np

# ---- remap: hand-built maps ------------------------------------------------------------------------------------------------
SRC_SIZES = ((1, 1), (2, 2), (7, 5), (300, 3))                    # (sw, sh)
DST_SIZES = ((1, 1), (255, 2), (256, 1), (257, 2), (300, 3))      # (W, H): either side of the kernel's 256-wide block
UNREPRESENTABLE = (float("nan"), float("inf"), float("-inf"), 3e9, -3e9, 2.0 ** 26, -2.0 ** 26 - 8, 2.0 ** 31 / 32)
HUGE_BUT_REPRESENTABLE = (-2.0 ** 26, 2.0 ** 26 - 4)              # * 32 = INT_MIN and the largest float below 2^31: far outside, no rule needed


def source(sw, sh, seed=1, top=255):
    """Random pixels in 1..top: never 0, so a tap that wrongly reads the source instead of the border shows."""
    return np.random.default_rng(seed).integers(1, top + 1, (sh, sw)).astype(np.uint8)


def _grid(xs, ys):
    mx, my = np.meshgrid(np.asarray(xs, np.float32), np.asarray(ys, np.float32))
    return np.ascontiguousarray(mx), np.ascontiguousarray(my)


def sweep_cases():
    """Every source size into every destination size: coordinates in 1/64 steps (half of them round-half-even ties) from three
    pixels before the source to two past it."""
    out = []
    for k, (sw, sh) in enumerate(SRC_SIZES):
        for m, (W, H) in enumerate(DST_SIZES):
            rng = np.random.default_rng(100 + 10 * k + m)
            mx = (rng.integers(-3 * 64, (sw + 2) * 64 + 1, (H, W)) / 64.0).astype(np.float32)
            my = (rng.integers(-3 * 64, (sh + 2) * 64 + 1, (H, W)) / 64.0).astype(np.float32)
            out.append(("sweep_%dx%d_to_%dx%d" % (sw, sh, W, H), source(sw, sh, 7 + k), mx, my))
    return out


def phase_case():
    """All 32 x 32 (fx, fy) phases at interior pixel (3, 2) of a 7x5 source."""
    mx, my = _grid([3 + f / 32.0 for f in range(32)], [2 + f / 32.0 for f in range(32)])
    return [("phases_32x32", source(7, 5, 3), mx, my)]


def border_cases():
    """ix on each of -2, -1, 0, sw-2, sw-1, sw crossed with the same for iy (all four corners among them), at fractions 0, 1/32, 1/2
    and 31/32: none, one, two or three of the four taps fall outside."""
    out = []
    for sw, sh in SRC_SIZES:
        xs = [p + f / 32.0 for p in (-2, -1, 0, sw - 2, sw - 1, sw) for f in (0, 1, 16, 31)]
        ys = [p + f / 32.0 for p in (-2, -1, 0, sh - 2, sh - 1, sh) for f in (0, 1, 16, 31)]
        out.append(("borders_%dx%d" % (sw, sh), source(sw, sh, 11), *_grid(xs, ys)))
    return out


def tie_cases():
    """Negative fractions and ties: v * 32 = -0.5 (-> 0), -1.5 (-> -2), -16, -32, -32.5 (-> -32), 32 k + 0.5 (-> 32 k) and
    32 k + 1.5 (-> 32 k + 2): round half to even, neither away from zero nor truncated; floor semantics of >> 5 and & 31 below zero."""
    out = []
    for sw, sh in ((7, 5), (2, 2)):
        def line(n):
            return [-1 / 64.0, -3 / 64.0, -0.5, -1.0, -1 - 1 / 64.0] + [k + d / 64.0 for k in range(n) for d in (1, 3)]
        out.append(("ties_%dx%d" % (sw, sh), source(sw, sh, 13), *_grid(line(sw), line(sh))))
    return out


def unrepresentable_cases():
    """NaN, +-inf, +-3e9, 2^26 = 2^31 / 32 and -2^26 - 8 in x alone, in y alone and in both, next to coordinates that land on source
    pixel (0, 0) (which is not 0): every such pixel must be the border value.  -2^26 and 2^26 - 4 are representable and simply far
    outside."""
    out = []
    for sw, sh in ((7, 5), (1, 1)):
        good = (0.0, 0.25, 0.5)
        bad = UNREPRESENTABLE + HUGE_BUT_REPRESENTABLE
        pairs = ([(g, g) for g in good] + [(b, g) for b in bad for g in good] + [(g, b) for b in bad for g in good] +
                 [(a, b) for a in bad for b in bad])                       # the first three: controls that do sample the source
        mx = np.array([[p[0] for p in pairs]], np.float32)
        my = np.array([[p[1] for p in pairs]], np.float32)
        out.append(("unrepresentable_%dx%d" % (sw, sh), source(sw, sh, 17), mx, my))
    return out


def remap_cases():
    """-> [(name, src uint8 [sh][sw], mapx float32 [H][W], mapy float32 [H][W])]"""
    return sweep_cases() + phase_case() + border_cases() + tie_cases() + unrepresentable_cases()


# ---- maps: calibrations ----------------------------------------------------------------------------------------------------
MAP_SIZES = ((1, 1), (257, 2), (320, 180), (333, 187))
WALK_SIZES = ((320, 180), (333, 187), (640, 360), (1280, 720))


def _rodrigues(om):
    om = np.asarray(om, np.float64)
    th = np.linalg.norm(om)
    k = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def synthetic_calibrations():
    """-> [(K[9], D[5], R[9], P[12])]: all five distortion coefficients non-zero and pairwise different (in magnitude too), fx != fy,
    R not the identity, P's focal lengths and principal point unlike K's — a swap of p1 / p2, of k2 / k3 or of fx / fy moves the map
    by far more than a float ulp."""
    out = []
    for fx, fy, cx, cy, D, om, pf, pc in (
            (412.5, 431.25, 318.0, 181.5, (-0.31, 0.12, 0.0013, -0.0027, -0.021), (0.010, -0.020, 0.005), (300.0, 310.0), (160.5, 92.25)),
            (700.0, 655.0, 301.0, 250.0, (0.21, -0.35, -0.004, 0.0015, 0.09), (-0.03, 0.015, -0.02), (505.5, 498.0), (170.0, 88.0)),
            (250.5, 262.0, 170.0, 85.0, (-0.12, 0.03, 0.011, 0.007, -0.002), (0.002, 0.04, 0.01), (199.0, 207.5), (150.0, 101.0)),
            (1033.0, 1012.0, 640.0, 350.0, (0.05, 0.6, -0.0008, -0.0031, -1.2), (-0.015, -0.01, 0.03), (810.0, 790.0), (166.0, 93.5))):
        K = [fx, 0, cx, 0, fy, cy, 0, 0, 1]
        P = [pf[0], 0, pc[0], -37.5, 0, pf[1], pc[1], 0, 0, 0, 1, 0]
        out.append((K, list(D), list(_rodrigues(om).ravel()), P))
    return out


def shipped_calibrations(node, W, H):
    """Both eyes of the shipped rig, rectified for a W x H image (sizes below the node's 320x180 use that size's rectification)."""
    c = node.stereo_calib()
    r = node.stereo_rectify(c, max(W, 320), max(H, 180))
    return [(list(c.K1), list(c.D1), list(r.R1), list(r.P1)), (list(c.K2), list(c.D2), list(r.R2), list(r.P2))]


def cancelling_calibrations(per_calibration=12):
    """-> [(K, D, R, P, W, H)]: the synthetic calibrations with the principal point (u0, v0) of K tuned so that the LAST pixel
    (W - 1, H - 1) of a W x H map maps to exactly (0, 0): u0 = -(fx * t) with t that pixel's own distorted coordinate, so the final
    fx * t + u0 cancels.  Everywhere else a float32 entry absorbs a last-bit change of the double behind it (a 1 in ~1e9 chance to
    show); here the entry is the bare rounding residue, and float32 resolves it: a kernel whose a * b + c was contracted to an
    fma writes ~1e-14 instead of 0.  Which contractions these maps see is asserted in tests/test_rectify.py."""
    import frontend_def as fd
    rng = np.random.default_rng(5)
    out = []
    for K, D, R, P in synthetic_calibrations():
        for _ in range(per_calibration):
            j0, i0 = int(rng.integers(40, 333)), int(rng.integers(20, 187))
            K0 = list(K); K0[2] = 0.0; K0[5] = 0.0
            u, v = fd.undistort_pixel(K0, D, R, P, j0, i0)              # fx * t + 0: the rounded product itself
            K1 = list(K); K1[2] = -float(u); K1[5] = -float(v)
            out.append((K1, D, R, P, j0 + 1, i0 + 1))
    return out


# ---- JPEG: synthetic coefficients ------------------------------------------------------------------------------------------
JPEG_SIZES = ((1, 1), (8, 8), (9, 9), (17, 8), (264, 8), (8, 264))      # the last two: 33 blocks, one more than a workgroup takes
DENSE_AMPLITUDE, DENSE_QMAX = 150, 24          # chosen on the CPU: see jpeg_pools


def _single(pos, v):
    b = np.zeros(64, np.int64); b[pos] = v
    return b.reshape(8, 8)


def jpeg_pools():
    """-> [(name, quant [8][8], blocks [n][8][8] quantised, fits_int32)].
    q1 / q255: DC alone at +-1, +-1023, +-2047 and a single +-1023 coefficient at each of the 64 positions, every quantiser 1
    resp. 255.  1023 * 255 = 260865 does not fit a 32-bit inverse DCT at ANY position (DC: pass 1 gives 4 * 260865, and pass 2
    shifts that left by 13 bits: 8.5e9), so that pool alone is compared with the exact int64 definition without the int32
    assertion — which is what libjpeg computes (jpeg_def).
    dense: every coefficient uniform in +-DENSE_AMPLITUDE, quantisers uniform in 1..DENSE_QMAX: values before range limiting spread
    past +-1500 while every 32-bit intermediate still fits (asserted by tests/test_jpeg.py)."""
    dc_alone = [_single(0, v) for v in (1, -1, 1023, -1023, 2047, -2047)]
    singles = [_single(p, s * 1023) for p in range(64) for s in (1, -1)]
    rng = np.random.default_rng(33)
    dense = rng.integers(-DENSE_AMPLITUDE, DENSE_AMPLITUDE + 1, (150, 8, 8))
    return [("q1", np.full((8, 8), 1), np.array(dc_alone + singles), True),
            ("q255", np.full((8, 8), 255), np.array(dc_alone + singles), False),
            ("dense", rng.integers(1, DENSE_QMAX + 1, (8, 8)), dense, True)]


def jpeg_frames():
    """-> [(name, W, H, quant, coef [bh][bw][8][8], fits_int32)]: each pool dealt into frames of the six sizes in turn until it is used
    up (the last frame wraps round to the pool's start).  Within a frame the blocks are ordered by DC value: the Annex K table
    has no code for a DC difference beyond 11 bits, and +2047 next to -2047 would need 12."""
    out = []
    for name, quant, blocks, fits in jpeg_pools():
        at, k = 0, 0
        while at < len(blocks):
            W, H = JPEG_SIZES[k % len(JPEG_SIZES)]
            bw, bh = (W + 7) // 8, (H + 7) // 8
            take = blocks[np.arange(at, at + bw * bh) % len(blocks)]
            take = take[np.argsort(take[:, 0, 0], kind="stable")]
            out.append(("%s_%d_%dx%d" % (name, k, W, H), W, H, quant, take.reshape(bh, bw, 8, 8), fits))
            at += bw * bh; k += 1
    return out

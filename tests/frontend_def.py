"""The camera front end restated in numpy: initUndistortRectifyMap and remap (INTER_LINEAR, constant 0 border) as the node uses them
(point_cloud.cpp:440, :481, :553-554).  TEST INFRASTRUCTURE: the checker of tests/test_gpu_frontend.py and tests/test_rectify.py.
Shares no code with oracle/node_oracle.cpp or csrc/scan.hip; every operation is a separate, correctly rounded numpy operation
(numpy never contracts a*b+c), so `undistort_map` is the formula in IEEE double, operation by operation."""
import numpy as np


def inverse_3x3(M):
    """Cofactor inverse of a 3x3 (flat, row major) in the order jn_init_undistort_rectify_map / orc_init_undistort_rectify_map use."""
    M = [np.float64(v) for v in M]
    c00 = M[4] * M[8] - M[5] * M[7]
    c01 = M[5] * M[6] - M[3] * M[8]
    c02 = M[3] * M[7] - M[4] * M[6]
    idet = np.float64(1.0) / (M[0] * c00 + M[1] * c01 + M[2] * c02)
    return [c00 * idet, (M[2] * M[7] - M[1] * M[8]) * idet, (M[1] * M[5] - M[2] * M[4]) * idet,
            c01 * idet, (M[0] * M[8] - M[2] * M[6]) * idet, (M[2] * M[3] - M[0] * M[5]) * idet,
            c02 * idet, (M[1] * M[6] - M[0] * M[7]) * idet, (M[0] * M[4] - M[1] * M[3]) * idet]


def undistort_map(K, D, R, P, W, H, walk=False):
    """-> (mapx, mapy) float32 [H][W]: for every rectified pixel (j, i) the distorted source position.
    iR = inverse(P[:, :3] * R); ray = iR (j, i, 1); x, y = ray / w; radial k1 k2 k3 and tangential p1 p2; u = fx x'' + u0.
    walk=False evaluates the column term as j * iR[0] (the kernel, the oracle); walk=True starts every row at i * iR[1] + iR[2]
    and adds iR[0] once per column, as OpenCV's loop does (`_x += ir[0]`)."""
    K, D, R, P = (np.asarray(a, np.float64).ravel() for a in (K, D, R, P))
    M = [P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j] + P[4 * i + 2] * R[6 + j] for i in range(3) for j in range(3)]
    iR = inverse_3x3(M)
    k1, k2, p1, p2, k3 = D[:5]
    fx, fy, u0, v0 = K[0], K[4], K[2], K[5]
    j = np.arange(W, dtype=np.float64)[None, :]
    i = np.arange(H, dtype=np.float64)[:, None]

    def ray(a, b, c):
        if not walk:
            return j * a + i * b + c
        steps = np.empty((H, W), np.float64)
        steps[:, :1] = i * b + c
        steps[:, 1:] = a
        return np.add.accumulate(steps, axis=1)          # sequential: out[j] = out[j - 1] + a

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        _x, _y, _w = ray(iR[0], iR[1], iR[2]), ray(iR[3], iR[4], iR[5]), ray(iR[6], iR[7], iR[8])
        w = 1.0 / _w
        x = _x * w
        y = _y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
        return u.astype(np.float32), v.astype(np.float32)


def fixed_point(v):
    """-> (s int64, representable bool): the 1/32-pixel coordinate rint(float32(v) * float32(32)), ties to even.  A coordinate whose
    rounded value is not finite or lies outside int32 is unrepresentable (s is 0 there and must not be used)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.asarray(v, np.float32) * np.float32(32))
        ok = np.isfinite(r) & (r >= np.float32(-2.0 ** 31)) & (r < np.float32(2.0 ** 31))
    return np.where(ok, r, 0).astype(np.int64), ok


def remap(src, mapx, mapy):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit pixels: ix = s >> 5 and f = s & 31 (floor semantics for negatives), four
    taps with weights (32 - fx | fx) * (32 - fy | fy), a tap outside the source is 0, result (acc + 512) >> 10.
    Unrepresentable coordinate (see fixed_point) in x or y: the pixel is the border value 0 — OpenCV on x86 gets there through
    cvRound -> INT_MIN -> saturated short -32768, which lies outside every image."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    sx, okx = fixed_point(mapx)
    sy, oky = fixed_point(mapy)
    ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < sw) & (yy >= 0) & (yy < sh)
        return np.where(inside, src[np.clip(yy, 0, sh - 1), np.clip(xx, 0, sw - 1)].astype(np.int64), 0)

    acc = ((32 - fx) * (32 - fy) * tap(ix, iy) + fx * (32 - fy) * tap(ix + 1, iy) +
           (32 - fx) * fy * tap(ix, iy + 1) + fx * fy * tap(ix + 1, iy + 1))
    return np.where(okx & oky, (acc + 512) >> 10, 0).astype(np.uint8)


# ---- what a contracted kernel would compute: used to PROVE that the map tests can see a contraction, never as a reference ----------
def fma(a, b, c):
    """a * b + c with one rounding (exact rational arithmetic, then the correctly rounded conversion)."""
    from fractions import Fraction
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


FMA_SITES = ("ray_x_j", "ray_x_i", "ray_y_j", "ray_y_i", "ray_w_j", "ray_w_i", "r2_x", "r2_y", "kr_k3", "kr_k2", "kr_k1",
             "u_xkr", "u_p1", "u_p2", "u_fx", "v_ykr", "v_p1", "v_p2", "v_fy")


def undistort_pixel(K, D, R, P, j, i, site=None):
    """-> (u, v) float64 of one pixel, the formula of undistort_map operation by operation (site=None gives its very doubles).
    `site` names ONE multiply whose product goes unrounded into the add that follows it (FMA_SITES), as a compiler that contracts
    a * b + c would emit; 2 * x is exact and has no site."""
    K, D, R, P = (np.asarray(a, np.float64).ravel() for a in (K, D, R, P))
    M = [P[4 * a] * R[b] + P[4 * a + 1] * R[3 + b] + P[4 * a + 2] * R[6 + b] for a in range(3) for b in range(3)]
    iR = inverse_3x3(M)
    k1, k2, p1, p2, k3 = D[:5]
    fx, fy, u0, v0 = K[0], K[4], K[2], K[5]
    fj, fi = np.float64(j), np.float64(i)

    def mad(name, a, b, c):                                   # a * b + c, contracted iff this is the chosen site
        return fma(a, b, c) if site == name else a * b + c

    def ray(name, a, b, c):
        if site == name + "_j":
            return fma(fj, a, fi * b) + c
        return mad(name + "_i", fi, b, fj * a) + c

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        _x, _y, _w = ray("ray_x", iR[0], iR[1], iR[2]), ray("ray_y", iR[3], iR[4], iR[5]), ray("ray_w", iR[6], iR[7], iR[8])
        w = 1.0 / _w
        x = _x * w
        y = _y * w
        x2 = x * x
        y2 = y * y
        r2 = fma(x, x, y2) if site == "r2_x" else mad("r2_y", y, y, x2)
        _2xy = 2 * x * y
        kr = mad("kr_k1", mad("kr_k2", mad("kr_k3", k3, r2, k2), r2, k1), r2, np.float64(1))
        tu = fma(x, kr, p1 * _2xy) if site == "u_xkr" else mad("u_p1", p1, _2xy, x * kr)
        tu = mad("u_p2", p2, r2 + 2 * x2, tu)
        tv = fma(y, kr, p1 * (r2 + 2 * y2)) if site == "v_ykr" else mad("v_p1", p1, r2 + 2 * y2, y * kr)
        tv = mad("v_p2", p2, _2xy, tv)
        return mad("u_fx", fx, tu, u0), mad("v_fy", fy, tv, v0)

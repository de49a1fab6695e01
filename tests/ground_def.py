"""The definition of the ground-plane estimator (include/jn_ground.h), restated in plain numpy / Python integers: sampling, planes, gate,
scores, pick, sums, host solve, geometry, alignment.  The checker of tests/test_ground_api.py and tests/test_gpu_ground.py; slow on
purpose, and it shares no code with jackal_navigation_amd/ground.py."""
import math

import numpy as np

F32, I16, I16_SUB = 0, 1, 2
MAX_Q = 16 * 4096
OK, FEW_SUPPORT = 0, 1


def mix32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def to_q(disp, fmt, min_disp):
    """-> (q int64, valid bool), the shape of disp."""
    if fmt == F32:
        d = np.asarray(disp, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.rint(np.float32(16) * d)                              # float32; numpy's rint rounds half to even
            valid = np.isfinite(d) & (t >= np.float32(16 * min_disp)) & (t <= np.float32(MAX_Q))
        q = np.where(valid, t, 0).astype(np.int64)
    else:
        q = np.asarray(disp, np.int16).astype(np.int64) * (16 if fmt == I16 else 1)
        valid = (q >= 16 * min_disp) & (q <= MAX_Q)
    return q, valid


def q16(v):
    """llrint(16 * v * 65536): round half to even on the double product."""
    return int(np.rint(np.float64(16.0) * np.float64(v) * np.float64(65536.0)))


def hypotheses(q, valid, f, gp):
    """q / valid of frame f -> K rows (A, B, C, E), zero for VOID."""
    rw, rh = gp.roi_x1 - gp.roi_x0, gp.roi_y1 - gp.roi_y0
    bq, aq = q16(gp.beta_min), q16(gp.alpha_max)
    out = np.zeros((gp.hypotheses, 4), np.int64)
    for k in range(gp.hypotheses):
        pts = []
        for j in range(3):
            for t in range(8):
                h = mix32(gp.seed ^ mix32((((((f * 1024 + k) & 0xffffffff) * 3 + j) & 0xffffffff) * 8 + t) & 0xffffffff))
                x = gp.roi_x0 + (((h & 0xffff) * rw) >> 16)
                y = gp.roi_y0 + (((h >> 16) * rh) >> 16)
                if valid[y, x]:
                    pts.append((x, y, int(q[y, x])))
                    break
            else:
                break
        if len(pts) < 3:
            continue
        (x0, y0, q0), (x1, y1, q1), (x2, y2, q2) = pts
        dx1, dy1, dq1, dx2, dy2, dq2 = x1 - x0, y1 - y0, q1 - q0, x2 - x0, y2 - y0, q2 - q0
        A, B, C = dy1 * dq2 - dq1 * dy2, dq1 * dx2 - dx1 * dq2, dx1 * dy2 - dy1 * dx2
        if C == 0:
            continue
        sgn = 1 if C > 0 else -1
        if not (-B * sgn * 65536 >= bq * abs(C) and abs(A) * 65536 <= aq * abs(C)):
            continue
        assert max(abs(A), abs(B), abs(C)) < 2 ** 31
        out[k] = (A, B, C, -(A * x0 + B * y0 + C * q0))
    return out


def region(gp, a):
    return a[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1]


def residual_inliers(q, valid, gp, hyp):
    """bool mask over the region of the inliers of one hypothesis."""
    A, B, C, E = (int(v) for v in hyp)
    if C == 0:
        return np.zeros_like(region(gp, valid))
    ys, xs = np.mgrid[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1].astype(np.int64)
    r = A * xs + B * ys + C * region(gp, q) + E
    return region(gp, valid) & (np.abs(r) <= gp.tol_q * abs(C))


def scores(q, valid, gp, hyps):
    return np.array([int(residual_inliers(q, valid, gp, h).sum()) for h in hyps], np.int32)


def pick(sc):
    return int(np.argmax(sc))                                            # the first of the largest


def sums(q, valid, gp, hyp):
    """-> ([N, Sx, Sy, Sq, Sxx, Sxy, Syy, Sxq, Syq, Sqq] as Python integers, valid count)."""
    m = residual_inliers(q, valid, gp, hyp)
    ys, xs = np.mgrid[gp.roi_y0:gp.roi_y1, gp.roi_x0:gp.roi_x1].astype(np.int64)
    x, y, qq = xs[m], ys[m], region(gp, q)[m]
    s = [int(m.sum()), x.sum(), y.sum(), qq.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), (x * qq).sum(), (y * qq).sum(), (qq * qq).sum()]
    return [int(v) for v in s], int(region(gp, valid).sum())


def solve(sp, S, valid, min_inliers=0, min_inlier_frac=0.0):
    """-> dict(status, a, b, c, rms, n_cam, height_m) from the ten sums, by the header's rules."""
    zero = dict(status=FEW_SUPPORT, a=0.0, b=0.0, c=0.0, rms=0.0, n_cam=np.zeros(3), height_m=0.0)
    N, Sx, Sy, Sq, Sxx, Sxy, Syy, Sxq, Syq, Sqq = (int(v) for v in S)
    if N < 3 or N < min_inliers or N < min_inlier_frac * valid:
        return zero
    Mxx, Mxy, Myy = float(N * Sxx - Sx * Sx), float(N * Sxy - Sx * Sy), float(N * Syy - Sy * Sy)
    Mxq, Myq, Mqq = float(N * Sxq - Sx * Sq), float(N * Syq - Sy * Sq), float(N * Sqq - Sq * Sq)
    det = Mxx * Myy - Mxy * Mxy
    if not det > 0:
        return zero
    aq, bq = (Mxq * Myy - Myq * Mxy) / det, (Myq * Mxx - Mxq * Mxy) / det
    cq = (Sq - aq * Sx - bq * Sy) / N
    a, b, c = aq / 16, bq / 16, cq / 16
    rms = math.sqrt(max(0.0, Mqq - aq * Mxq - bq * Myq)) / N / 16
    Q = np.array(sp.Q, np.float64).reshape(4, 4)
    pd = np.array([a, b, -1.0, c - a * sp.crop_offset_x - b * sp.crop_offset_y])
    p3 = np.linalg.solve(Q.T, pd)
    p3 = p3 / np.linalg.norm(p3[:3])
    if p3[3] < 0:
        p3 = -p3
    return dict(status=OK, a=a, b=b, c=c, rms=rms, n_cam=p3[:3].copy(), height_m=float(p3[3]))


def frame(disp, fmt, f, gp, sp=None):
    """Everything the definition says about frame f: dict(hyps, scores, best, sums, valid) and, with sp, the solved plane."""
    q, valid = to_q(disp, fmt, gp.min_disp)
    hy = hypotheses(q, valid, f, gp)
    sc = scores(q, valid, gp, hy)
    best = pick(sc)
    S, nv = sums(q, valid, gp, hy[best])
    out = dict(hyps=hy, scores=sc, best=best, sums=S, valid=nv)
    if sp is not None:
        out.update(solve(sp, S, nv, gp.min_inliers, gp.min_inlier_frac))
    return out


def align(n_cam, height_m, XR0, XT0):
    """-> (XR, XT, tilt_deg): Rodrigues about n x u0, u0 = XR0^T e_z."""
    XR0 = np.asarray(XR0, np.float64).reshape(3, 3)
    n = np.asarray(n_cam, np.float64) / np.linalg.norm(n_cam)
    u = XR0[2] / np.linalg.norm(XR0[2])
    ax = np.cross(n, u)
    s, c = np.linalg.norm(ax), float(n @ u)
    R = np.eye(3)
    if s >= 1e-15:
        k = ax / s
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + s * Kx + (1 - c) * (Kx @ Kx)
    return XR0 @ R, np.array([XT0[0], XT0[1], height_m]), math.degrees(math.atan2(s, c))


def joint(sp, planes_sums):
    """The joint fit of several frames: the sums added, solved once."""
    S = [sum(int(p[i]) for p in planes_sums) for i in range(10)]
    return solve(sp, S, 0)


# ---- geometry helpers for the tests: the disparity of a robot-frame floor ----

def floor_disparity(sp, XR, XT, W, H):
    """The exact disparity (float64, pixels) at every pixel of the robot-frame plane z = 0, for a camera with sp.Q and XR / XT:
    the plane n . cam + h = 0 with n = XR^T e_z, h = XT.z, pulled back through Q: pi_d = Q^T pi_3 on [x, y, d, 1]."""
    XR = np.asarray(XR, np.float64).reshape(3, 3)
    Q = np.array(sp.Q, np.float64).reshape(4, 4)
    pd = Q.T @ np.array([XR[2, 0], XR[2, 1], XR[2, 2], XT[2]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return -(pd[0] * (xs + sp.crop_offset_x) + pd[1] * (ys + sp.crop_offset_y) + pd[3]) / pd[2]


def rot_xyz(roll_deg, pitch_deg):
    """A small rotation of the robot frame: roll about x, then pitch about y."""
    r, p = math.radians(roll_deg), math.radians(pitch_deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    return Ry @ Rx

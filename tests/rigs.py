"""A table of rigs for the navigation tails: tests/test_scan_def.py and tests/test_gpu_rigs.py run every kernel behind a disparity map under
each of them.  TEST INFRASTRUCTURE.  A rig is a function (sp, W, H) that edits a jn_scan_params-shaped ctypes struct in place
(node.scan_params and oracle.scan_params have the same fields); REACHES says, per rig, what its scan must be seen doing (facts() of
the test's own maps), so a rig that silently stops reaching its path fails the test that uses it."""
import math

import numpy as np

import costmap_def as cd

BASE = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])      # camera z forward -> robot x, camera x right -> robot -y, camera y down -> robot -z
STRIP = 16                                                          # rows one thread of k_scan / k_costmap_accumulate / k_spx_accumulate walks


def Rx(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[1., 0., 0.], [0., c, -s], [0., s, c]])


def Ry(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]])


def Rz(deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])


def _frame(sp, XR, XT):
    sp.XR[:] = np.asarray(XR, np.float64).reshape(-1).tolist()
    sp.XT[:] = [float(v) for v in XT]


def default(sp, W, H):
    """The shipped rig: the control."""


def pitched_yawed_rolled(sp, W, H):
    """Bins and cells change along a column; the field of view is seen from one side."""
    _frame(sp, Rz(40) @ Ry(25) @ Rx(8) @ BASE, (0.1, -0.05, 0.6))


def rear_fov360(sp, W, H):
    """atan2 with X < 0 on both sides of +-pi; with pi_approx = 3.1415 the bearings next to +-pi give deg beyond +-180: rejected.
    Only a bearing within 9.3e-5 rad of +-pi does that — a hundredth of a pixel from the principal point's column at these sizes — so the
    principal point is put on column W // 2, whose pixels have camera x = 0 and land on +-pi to the last bits of sin(180 deg)."""
    _frame(sp, Rz(180) @ BASE, (-0.2, 0.0, 0.3))
    sp.Q[3] = -float(W // 2)
    sp.fov_deg, sp.bins = 360.0, 64


def rear_minus_pi(sp, W, H):
    """rear_fov360 turned the other way round: sin(-180 deg) puts column W // 2 on -pi, where deg < -180 gives kf >= bins."""
    rear_fov360(sp, W, H)
    _frame(sp, Rz(-180) @ BASE, (-0.2, 0.0, 0.3))


def rolled90(sp, W, H):
    """A row of the image is a column of the world: every pixel of a strip is its own bin / cell; the largest LDS bin array."""
    _frame(sp, Rx(90) @ BASE, (0.0, 0.0, 0.5))
    sp.fov_deg, sp.bins = 120.0, 1024


def ideal_integer_pp(sp, W, H):
    """Y == 0 exactly in column W // 2 (atan2(0, X)); the odd bin count keeps that bearing off a bin edge."""
    _frame(sp, BASE, (0.0, 0.0, 0.25))
    sp.Q[3], sp.Q[7] = -float(W // 2), -float(H // 2)
    sp.bins, sp.pi_approx = 91, math.pi


def tweak_w0(sp):
    """Disparity 7 gets homogeneous w = Q[14] * 7 + Q[15] = 0 exactly (the other terms of that row are 0).  The one edit of the rig the
    costmap, sub-pixel and local-map tests make on their own."""
    sp.Q[15] = -(sp.Q[14] * 7.0)
    return sp


def flipped_baseline_w0(sp, W, H):
    """The other sign convention of Tx; w = 0 at d = 7 and of either sign around it: points behind the camera, and at d = 6 and 8 ranges
    of f * B metres and beyond (13.6 m at width 200, 16 times that one sub-pixel step from w = 0; hundreds of metres at full size)."""
    sp.Q[14] = -sp.Q[14]
    sp.Q[11] = -sp.Q[11]
    tweak_w0(sp)


def fisheye_short_base_bins1(sp, W, H):
    """One bin; a flat ground model (tan = 0); points a few millimetres away."""
    sp.Q[11] *= 0.35
    sp.Q[14] *= 4.0
    sp.fov_deg, sp.bins = 170.0, 1
    sp.gp_angle_thresh, sp.gp_dist_thresh = 0.0, 0.3


def cropped(sp, W, H):
    """The default rig on a window cut out of a larger frame: both crop offsets enter the reprojection."""
    sp.crop_offset_x, sp.crop_offset_y = 37, 11


def gp_far(sp, W, H):
    """The default rig with only the first branch of the ground test."""
    sp.gp_dist_thresh = 1e9


def gp_steep(sp, W, H):
    """The default rig with only the second branch of the ground test; the lower rows of the table all go through the 256 -> 0 wrap."""
    sp.gp_angle_thresh, sp.gp_dist_thresh = math.radians(60.0), -1.0


def ground_boundary(sp, W, H):
    """ideal_integer_pp with a flat ground model whose height is the camera's own: row H // 2 has camera y = 0 exactly, so every point of
    it has Z = XT[2] = gp_height_thresh to the bit, for every disparity — ON the boundary of the second branch of the ground test (the
    first never runs: gp_dist_thresh = -1), where `<` says obstacle and `<=` would say ground."""
    ideal_integer_pp(sp, W, H)
    sp.gp_angle_thresh, sp.gp_dist_thresh, sp.gp_height_thresh = 0.0, -1.0, sp.XT[2]


RIGS = [default, pitched_yawed_rolled, rear_fov360, rear_minus_pi, rolled90, ideal_integer_pp, flipped_baseline_w0, fisheye_short_base_bins1, cropped, gp_far, gp_steep, ground_boundary]
NAMES = [r.__name__ for r in RIGS]
BY_NAME = {r.__name__: r for r in RIGS}
SEES_A_FLOOR = ["default", "pitched_yawed_rolled", "ideal_integer_pp", "fisheye_short_base_bins1"]


def apply(name, sp, W, H):
    BY_NAME[name](sp, W, H)
    return sp


def _second_branch_height(sp, X):
    """The height the second branch of the ground test compares Z with: costmap_def.is_ground's expression."""
    return sp.gp_height_thresh + math.tan(sp.gp_angle_thresh) * (X - sp.gp_dist_thresh)


def facts(sp, disp, lut, valid=None):
    """What the cloud-flavour scan (valid, w != 0, not ground) of the maps disp [n][H][W] (pixels; u8 or float) and the table
    lut [H][W][2] do under sp: the numbers REACHES looks at.  valid [n][H][W]: disp >= 2 when not given.  Everything from
    tests/costmap_def.py's expressions, as tests/scan_def.py."""
    n, H, W = disp.shape
    f = dict(strip_bin_changes=0, strip_bins_max=0, x_negative=0, th_above_3=0, th_below_minus_3=0, deg_beyond_180=0, y_zero_mid_column=0,
             w_zero=0, w_positive=0, w_negative=0, r_max=0.0, r_min=1e9, binned=0, left_of_fan=0, right_of_fan=0, first_branch=0,
             second_branch=0, ground_first=0, ground_second=0, on_boundary_second=0, lut_on_boundary_second=0, lut_zero=int((lut[..., 0] == 0).sum()), lut_rows_all_zero=int((lut[..., 0] == 0).all(axis=1).sum()),
             lut_z_negative=0, f_times_b=abs(sp.Q[11] / sp.Q[14]) if sp.Q[14] else 0.0, bins_hit=set(), crop=(int(sp.crop_offset_x), int(sp.crop_offset_y)))
    for idx, m in enumerate(disp):
        X, Y, Z, ok = cd.reproject(sp, m)
        v = (m >= 2) if valid is None else valid[idx]
        w = sp.Q[14] * m.astype(np.float64) + sp.Q[15]                                  # the rigs here keep Q[12] = Q[13] = 0
        f["w_zero"] += int((v & ~ok).sum())
        ground = cd.is_ground(sp, X, Z)
        cand = v & ok
        f["first_branch"] += int((cand & (X < sp.gp_dist_thresh)).sum()); f["second_branch"] += int((cand & ~(X < sp.gp_dist_thresh)).sum())
        f["ground_first"] += int((cand & ground & (X < sp.gp_dist_thresh)).sum()); f["ground_second"] += int((cand & ground & ~(X < sp.gp_dist_thresh)).sum())
        with np.errstate(all="ignore"):
            f["on_boundary_second"] += int((cand & ~(X < sp.gp_dist_thresh) & (Z == _second_branch_height(sp, X))).sum())
        take = cand & ~ground
        f["w_positive"] += int((take & (w > 0)).sum()); f["w_negative"] += int((take & (w < 0)).sum())
        with np.errstate(all="ignore"):
            th = np.arctan2(Y, X)
            deg = th * 180. / sp.pi_approx
            r = np.sqrt(Y * Y + X * X)
            kf = np.floor(sp.bins * (sp.fov_deg / 2. + -deg) / sp.fov_deg)
        inside = take & (kf >= 0) & (kf < sp.bins)
        f["x_negative"] += int((take & (X < 0)).sum())
        f["th_above_3"] += int((take & (th > 3.0)).sum()); f["th_below_minus_3"] += int((take & (th < -3.0)).sum())
        f["deg_beyond_180"] += int((take & (np.abs(deg) > 180.0)).sum())
        f["y_zero_mid_column"] += int((take[:, W // 2] & (Y[:, W // 2] == 0.0)).sum())
        f["left_of_fan"] += int((take & (kf < 0)).sum()); f["right_of_fan"] += int((take & (kf >= sp.bins)).sum())
        f["binned"] += int(inside.sum())
        if take.any():
            f["r_max"] = max(f["r_max"], float(r[take].max())); f["r_min"] = min(f["r_min"], float(r[take].min()))
        f["bins_hit"] |= set(np.unique(kf[inside]).astype(np.int64).tolist())
        k = np.where(inside, kf, -1).astype(np.int64)
        for j0 in range(0, H, STRIP):                                                  # per column: the bins of one thread's strip, in row order
            s = k[j0:j0 + STRIP]
            for col in range(W):
                c = s[:, col][s[:, col] >= 0]
                if c.size > 1:
                    ch = int((c[1:] != c[:-1]).sum())
                    f["strip_bin_changes"] += ch
                    f["strip_bins_max"] = max(f["strip_bins_max"], ch + 1)
    Xl, Yl, Zl, okl = cd.reproject(sp, np.full((H, W), 3, np.uint8))
    f["lut_z_negative"] = int((okl & (Zl < 0)).sum())                                    # d = 3 alone: enough to say the Z < 0 test runs
    with np.errstate(all="ignore"):
        f["lut_on_boundary_second"] = int((okl & ~(Xl < sp.gp_dist_thresh) & (Zl == _second_branch_height(sp, Xl)) & (lut[..., 0] == 3)).sum())
    return f


# per rig: (what the row of the table says, as a predicate over facts) -- shapes with at least two strips and a full block of columns
REACHES = {
    "default": lambda f: f["binned"] > 0 and f["x_negative"] == 0,
    "pitched_yawed_rolled": lambda f: f["strip_bin_changes"] > 50 and f["binned"] > 0 and (f["left_of_fan"] > 0) != (f["right_of_fan"] > 0),
    "rear_fov360": lambda f: f["x_negative"] > 0 and f["th_above_3"] > 0 and f["th_below_minus_3"] > 0 and f["deg_beyond_180"] > 0
    and f["left_of_fan"] > 0,
    "rear_minus_pi": lambda f: f["x_negative"] > 0 and f["deg_beyond_180"] > 0 and f["right_of_fan"] > 0,
    "rolled90": lambda f: f["strip_bins_max"] >= 12 and max(f["bins_hit"]) >= 256 and f["lut_z_negative"] > 0,
    "ideal_integer_pp": lambda f: f["y_zero_mid_column"] > 0,
    # one disparity step from w = 0 (d = 6 or 8) the depth is f * B: 13.6 m at the first shape's width, whose u8 maps reach 16.4 m with the
    # lateral offset and whose sub-pixel maps, 1/16 of a step from w = 0, reach 119 m; hundreds of metres come with the full-size f
    "flipped_baseline_w0": lambda f: f["w_zero"] > 0 and f["w_positive"] > 0 and f["w_negative"] > 0 and f["x_negative"] > 0
    and f["r_max"] >= f["f_times_b"] > 13.0,
    "fisheye_short_base_bins1": lambda f: f["bins_hit"] == {0} and f["r_min"] < 0.02 and f["ground_second"] > 0,
    "cropped": lambda f: f["binned"] > 0 and f["crop"][0] != 0 and f["crop"][1] != 0,
    "gp_far": lambda f: f["first_branch"] > 0 and f["second_branch"] == 0 and f["ground_first"] > 0,
    "gp_steep": lambda f: f["second_branch"] > 0 and f["first_branch"] == 0 and f["ground_second"] > 0 and f["lut_rows_all_zero"] > 0,
    # a whole row of the maps and of the table's candidates on the boundary, none of them ground, and the table says so (3: the first candidate)
    "ground_boundary": lambda f: f["on_boundary_second"] >= 100 and f["lut_on_boundary_second"] >= 200 and f["first_branch"] == 0,
}


# ---- inputs: what both the definition's own test and the GPU tests feed the tails ----
SPRINKLED = (0, 1, 2, 3, 7, 254, 255)


def u8_maps(rng, n, H, W):
    """Noise over the whole range, faces of constant disparity (the runs the kernels keep in registers), and the values that decide a
    branch — 0 / 1 (invalid), 2 (the cloud's first), 3 (the table's first), 7 (w = 0 under flipped_baseline_w0), 254 / 255 — sprinkled in."""
    m = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    for f in range(n):
        for _ in range(10):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            m[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(3, 120)
    special = rng.random((n, H, W))
    for k, v in enumerate(SPRINKLED):
        m[(special >= 0.03 * k) & (special < 0.03 * (k + 1))] = v
    return m


def float_maps(rng, n, H, W):
    """Float maps as ELAS writes them: u8_maps' values with noise below the rounding step, ELAS's invalid values (-10, -1), and ties at
    k + 0.5 on both parities of k."""
    m = u8_maps(rng, n, H, W).astype(np.float64) + rng.uniform(-0.45, 0.45, (n, H, W))
    special = rng.random((n, H, W))
    m[special < 0.03] = -10.0
    m[(special >= 0.03) & (special < 0.05)] = -1.0
    ties = (special >= 0.05) & (special < 0.10)
    m[ties] = rng.integers(0, 256, (n, H, W))[ties] + 0.5
    return m.astype(np.float32)


def decisive_floats():
    """The values that decide convertTo(CV_8U): every k + 0.5, k +- 2^-10 and k + 0.5 +- 2^-10 for k in -2..256, +-0, denormals, ELAS's invalid values, the
    edges of the saturation."""
    k = np.arange(-2, 257, dtype=np.float64)
    v = np.concatenate([k + 0.5, k + 2.0 ** -10, k - 2.0 ** -10, k + 0.5 + 2.0 ** -10, k + 0.5 - 2.0 ** -10, [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, -1.0, -10.0, 255.49998, 255.5, 256.0, 1e9, -1e9]])
    return v.astype(np.float32)

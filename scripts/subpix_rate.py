"""What the sub-pixel navigation tail (include/jn_subpix.h) costs next to the reference-parity tail it stands beside, and what it buys:
    python3 scripts/subpix_rate.py [calls_per_region] [regions]
Rate: per disparity format (float, int16, int16 in 1/16 pixel), 1280x720 batch 32 and 1920x1080 batch 8, the synchronous jn_subpix_scan
and jn_subpix_costmap (initialisation + the one pass + finish) timed by HIP events over regions of `calls_per_region` calls after a
warm-up, next to jn_obstacle_scan_cloud + jn_obstacle_costmap(from_cloud = 1) on the mono8 maps of the same disparities (the same
obstacle rule, so the same pixels do the same work).  Every call ends in a stream synchronisation, so a region holds the launch and
wait overhead of its calls as well as the kernels: `per_call_ms` is what a caller pays.
Accuracy: fronto-parallel walls 1.0 / 1.6 / 3.0 / 5.0 m along the optical axis through the default rig at 320x180; the true fractional
disparity (a) rounded to mono8 into jn_obstacle_scan_cloud, (b) rounded to 1/16 pixel into jn_subpix_scan (JN_DISP_I16_SUB); the median
over the bins of |range - true range|, the true range from the unrounded disparity in double on the host.
Prints one JSON line."""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import costmap, node, subpix  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402

try:
    import torch
    HAVE_EVENTS = torch.cuda.is_available()
except Exception:  # pragma: no cover
    HAVE_EVENTS = False


def scene_q(sp, n, H, W, seed):
    """Disparities in 1/16 pixel of a scene the rig could see: the floor (robot Z = 0 through sp's Q, XR, XT), a wall 8 m along the
    optical axis where the floor is farther than that or above the horizon, ten fronto-parallel boxes standing on the floor, sub-pixel
    noise, 3 % invalid pixels."""
    rng = np.random.default_rng(seed)
    Q, XR, XT = list(sp.Q), list(sp.XR), list(sp.XT)
    x = (np.arange(W, dtype=np.float64)[None, :] + Q[3]) / Q[11]
    y = (np.arange(H, dtype=np.float64)[:, None] + Q[7]) / Q[11]
    den = XR[6] * x + XR[7] * y + XR[8]                            # robot Z of the ray per metre of camera z
    with np.errstate(divide="ignore"):
        zf = np.where(den < 0, -XT[2] / den, np.inf)               # camera z where the ray meets the floor
    base = np.minimum(zf, 8.0)
    q = np.empty((n, H, W), np.int64)
    for f in range(n):
        z = base.copy()
        for _ in range(10):
            w = int(rng.integers(W // 40, W // 8)); x0 = int(rng.integers(0, W - w)); y1 = int(rng.integers(H // 2, H)); h = int(rng.integers(H // 10, H // 2))
            zb = zf[y1 - 1, x0 + w // 2]
            if np.isfinite(zb):
                box = z[max(0, y1 - h):y1, x0:x0 + w]
                box[box > zb] = zb
        d = Q[11] / (Q[14] * z) + rng.normal(0.0, 0.08, (H, W))
        q[f] = np.rint(16.0 * d)
        q[f][rng.random((H, W)) < 0.03] = -160
    return q


def formats_of(q):
    u8 = np.clip(np.rint(q / 16.0), 0, 255).astype(np.uint8)              # round half to even, as jn_disparity_to_u8
    return {subpix.F32: (q / 16.0).astype(np.float32), subpix.I16: np.floor_divide(q + 8, 16).astype(np.int16), subpix.I16_SUB: q.astype(np.int16)}, u8


def region_ms(fn, calls):
    if HAVE_EVENTS:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e3


def rate(W, H, B, calls, regions):
    sp, cp = node.scan_params(W, H), costmap.costmap_params(from_cloud=1)
    maps, u8 = formats_of(scene_q(sp, B, H, W, 7))
    bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
    hits = DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)
    dU = DeviceArray.from_numpy(u8)

    def u8_scan():
        node.obstacle_scan_cloud(sp, B, dU.ptr, W, H, bins.ptr, meta.ptr)

    def u8_both():
        node.obstacle_scan_cloud(sp, B, dU.ptr, W, H, bins.ptr, meta.ptr)
        costmap.obstacle_costmap(sp, cp, B, dU.ptr, None, W, H, bins.ptr, hits.ptr, grid.ptr)

    def measure(fn):
        for _ in range(5):
            fn()
        return round(statistics.median(region_ms(fn, calls) for _ in range(regions)), 4)

    out = {"size": [W, H], "batch": B, "u8_scan_cloud_per_call_ms": measure(u8_scan), "u8_scan_cloud_plus_costmap_per_call_ms": measure(u8_both)}
    g8 = grid.numpy()
    out["u8_cells_occupied_frame0"] = int((g8[0] == 100).sum())
    names = {subpix.F32: "f32", subpix.I16: "i16", subpix.I16_SUB: "i16_sub"}
    for fmt, arr in maps.items():
        dD = DeviceArray.from_numpy(arr)
        fp = subpix.subpix_params(fmt)
        out["subpix_scan_%s_per_call_ms" % names[fmt]] = measure(lambda: subpix.subpix_scan(sp, fp, B, dD.ptr, W, H, bins.ptr, meta.ptr))
        out["subpix_costmap_%s_per_call_ms" % names[fmt]] = measure(
            lambda: subpix.subpix_costmap(sp, cp, fp, B, dD.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr))
        out["subpix_cells_occupied_frame0_%s" % names[fmt]] = int((grid.numpy()[0] == 100).sum())
        dD.free()
    return out


def true_ranges(sp, W, H, d):
    """bins of a map of constant (real-valued) disparity d, in double on the host."""
    Q, XR, XT = list(sp.Q), list(sp.XR), list(sp.XT)
    V0 = (np.arange(W, dtype=np.float64)[None, :] + sp.crop_offset_x) * np.ones((H, 1))
    V1 = (np.arange(H, dtype=np.float64)[:, None] + sp.crop_offset_y) * np.ones((1, W))
    pos = [Q[4 * r] * V0 + Q[4 * r + 1] * V1 + Q[4 * r + 2] * d + Q[4 * r + 3] for r in range(4)]
    cam = [pos[k] / pos[3] for k in range(3)]
    X, Y, Z = (XR[3 * r] * cam[0] + XR[3 * r + 1] * cam[1] + XR[3 * r + 2] * cam[2] + XT[r] for r in range(3))
    ground = np.where(X < sp.gp_dist_thresh, Z < sp.gp_height_thresh, Z < sp.gp_height_thresh + math.tan(sp.gp_angle_thresh) * (X - sp.gp_dist_thresh))
    x, y = X[~ground], Y[~ground]
    k = np.floor(sp.bins * (sp.fov_deg / 2. - np.arctan2(y, x) * 180. / sp.pi_approx) / sp.fov_deg)
    r = np.sqrt(y * y + x * x)
    ok = (k >= 0) & (k < sp.bins)
    out = np.full(sp.bins, 1e9)
    np.minimum.at(out, k[ok].astype(np.int64), r[ok])
    return out


def accuracy():
    W, H = 320, 180
    sp = node.scan_params(W, H)
    Q = list(sp.Q)
    fp = subpix.subpix_params(subpix.I16_SUB)
    bins = DeviceArray((1, sp.bins), np.float64); meta = DeviceArray((1, 4), np.float64)
    rows = []
    for dist in (1.0, 1.6, 3.0, 5.0):
        d = (Q[11] / dist - Q[15]) / Q[14]                       # camera z = Q[2][3] / (Q[3][2] d + Q[3][3])
        truth = true_ranges(sp, W, H, d)
        hit = truth < 1e9 - 1
        dU = DeviceArray.from_numpy(np.full((1, H, W), int(np.rint(d)), np.uint8))
        node.obstacle_scan_cloud(sp, 1, dU.ptr, W, H, bins.ptr, meta.ptr)
        coarse = bins.numpy()[0]
        dQ = DeviceArray.from_numpy(np.full((1, H, W), int(np.rint(16.0 * d)), np.int16))
        subpix.subpix_scan(sp, fp, 1, dQ.ptr, W, H, bins.ptr, meta.ptr)
        fine = bins.numpy()[0]
        both = hit & (coarse < 1e9 - 1) & (fine < 1e9 - 1)
        rows.append({"wall_m": dist, "true_disparity_px": round(d, 4), "u8_disparity": int(np.rint(d)), "q_sixteenths": int(np.rint(16.0 * d)),
                     "bins_compared": int(both.sum()), "median_true_range_m": round(float(np.median(truth[both])), 4),
                     "u8_median_range_error_m": round(float(np.median(np.abs(coarse[both] - truth[both]))), 4),
                     "subpix_median_range_error_m": round(float(np.median(np.abs(fine[both] - truth[both]))), 4)})
    return rows


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    regions = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    L = jn.load()
    print(json.dumps({
        "script": "scripts/subpix_rate.py", "timer": "HIP events" if HAVE_EVENTS else "host clock", "calls_per_region": calls, "regions": regions,
        "rate": [rate(1280, 720, 32, calls, regions), rate(1920, 1080, 8, calls, regions)],
        "accuracy": accuracy(),
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

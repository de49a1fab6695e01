"""What an update of the local obstacle map (include/jn_localmap.h) costs next to the single-frame sub-pixel costmap it stands on:
    python3 scripts/localmap_rate.py [calls_per_region] [regions]
Per disparity format (float, int16, int16 in 1/16 pixel), 1280x720 batch 32 and 1920x1080 batch 8, on scripts/subpix_rate.py's driving
scene (floor, a far wall, boxes on the floor, sub-pixel noise, 3 % invalid pixels): the synchronous jn_localmap_update (pose upload, clear
of the counts, the pass over the pixels, the fuse) with a 256 x 256 window of 5 cm cells and poses along a gentle arc, timed by HIP events
over regions of `calls_per_region` calls after a warm-up, next to jn_subpix_costmap on the same maps (which counts the obstacle pixels
only, and also does the scan).  Every call ends in a stream synchronisation, so a region holds the launch and wait overhead of its calls as
well as the kernels: `per_call_ms` is what a caller pays.  `floor_share` / `obstacle_share`: the fraction of a frame's pixels counted as
each, from the update's own count outputs (window cells only).
Prints one JSON line."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import costmap, localmap, node, subpix  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402
from subpix_rate import HAVE_EVENTS, formats_of, region_ms, scene_q  # noqa: E402


def rate(W, H, B, calls, regions):
    sp, cp = node.scan_params(W, H), costmap.costmap_params(from_cloud=1)
    maps, _ = formats_of(scene_q(sp, B, H, W, 7))
    poses = [(0.02 * k, 0.001 * k * k, 0.01 * k) for k in range(B)]
    bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
    hits = DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)

    def measure(fn):
        for _ in range(5):
            fn()
        return round(statistics.median(region_ms(fn, calls) for _ in range(regions)), 4)

    out = {"size": [W, H], "batch": B}
    names = {subpix.F32: "f32", subpix.I16: "i16", subpix.I16_SUB: "i16_sub"}
    for fmt, arr in maps.items():
        dD = DeviceArray.from_numpy(arr)
        fp = subpix.subpix_params(fmt)
        p = localmap.localmap_params(fmt)
        out["subpix_costmap_%s_per_call_ms" % names[fmt]] = measure(
            lambda: subpix.subpix_costmap(sp, cp, fp, B, dD.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr))
        with localmap.LocalMap(p, max_batch=B) as m:
            dO = DeviceArray((B, p.cells_y, p.cells_x), np.uint16); dF = DeviceArray((B, p.cells_y, p.cells_x), np.uint16)
            m.update(sp, poses, dD.ptr, W, H, dO.ptr, dF.ptr)
            o, f = dO.numpy().astype(np.int64), dF.numpy().astype(np.int64)
            out["obstacle_share_%s" % names[fmt]] = round(float(o.sum()) / (B * W * H), 4)
            out["floor_share_%s" % names[fmt]] = round(float(f.sum()) / (B * W * H), 4)
            out["localmap_update_%s_per_call_ms" % names[fmt]] = measure(lambda: m.update(sp, poses, dD.ptr, W, H))
            out["localmap_update_with_counts_%s_per_call_ms" % names[fmt]] = measure(lambda: m.update(sp, poses, dD.ptr, W, H, dO.ptr, dF.ptr))
            g = m.read()[1]
            out["cells_occupied_%s" % names[fmt]] = int((g == 100).sum())
            out["cells_free_%s" % names[fmt]] = int((g == 0).sum())
            dO.free(); dF.free()
        dD.free()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    regions = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    L = jn.load()
    print(json.dumps({
        "script": "scripts/localmap_rate.py", "timer": "HIP events" if HAVE_EVENTS else "host clock", "calls_per_region": calls, "regions": regions,
        "window": "256 x 256 cells of 0.05 m (the defaults)",
        "rate": [rate(1280, 720, 32, calls, regions), rate(1920, 1080, 8, calls, regions)],
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

"""What the local planner (include/jn_plan.h) costs next to the map update that feeds it:
    python3 scripts/plan_rate.py [calls_per_region] [regions]
The synchronous jn_clearance on 1 x 256 x 256 (the local map's default window), 1 x 512 x 512 and 32 x 128 x 128 (a costmap batch) at
radius 20, 64 and 255, on grids with 1 % obstacle cells, a few blocks of unknown cells and free cells elsewhere; one jn_plan_command
(rollout of the default 33 candidates x 20 steps, records back to the host, the choice) on the 256 x 256 field; and, in the same process
with the same timer, jn_localmap_update and jn_subpix_costmap on scripts/localmap_rate.py's 1280x720 batch-32 workload (1/16-pixel maps)
as the yardstick.  HIP events over regions of `calls_per_region` calls after a warm-up, the median of `regions` regions.  Every call ends
in a stream synchronisation, so a region holds the launch and wait overhead of its calls as well as the kernels: `per_call_ms` is what a
caller pays.  k_clearance has one form; every figure is that form's.
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
from jackal_navigation_amd import costmap, localmap, node, plan, subpix  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402
from subpix_rate import HAVE_EVENTS, formats_of, region_ms, scene_q  # noqa: E402


def measure(fn, calls, regions):
    for _ in range(5):
        fn()
    return round(statistics.median(region_ms(fn, calls) for _ in range(regions)), 4)


def grids(n, cy, cx, seed):
    rng = np.random.default_rng(seed)
    g = np.zeros((n, cy, cx), np.int8)
    for f in range(n):
        for _ in range(4):
            y0, x0 = int(rng.integers(0, cy)), int(rng.integers(0, cx))
            g[f, y0:y0 + 24, x0:x0 + 24] = -1
        g[f][rng.random((cy, cx)) < 0.01] = 100
    return g


def clearance_rates(calls, regions):
    out = []
    for n, cy, cx in ((1, 256, 256), (1, 512, 512), (32, 128, 128)):
        dG = DeviceArray.from_numpy(grids(n, cy, cx, 3)); dD = DeviceArray((n, cy, cx), np.uint16)
        row = {"grids": [n, cy, cx]}
        for R in (20, 64, 255):
            row["clearance_r%d_per_call_ms" % R] = measure(lambda: plan.clearance(dG.ptr, R, 0, n, cx, cy, dD.ptr), calls, regions)
        row["far_share_r255"] = round(float((dD.numpy() == plan.FAR).mean()), 4)
        out.append(row)
        dG.free(); dD.free()
    return out


def plan_rate(calls, regions):
    p = plan.plan_params()
    dG = DeviceArray.from_numpy(grids(1, 256, 256, 3)); dD = DeviceArray((1, 256, 256), np.uint16)
    plan.clearance(dG.ptr, 20, 0, 1, 256, 256, dD.ptr)
    with plan.Plan(p, 0.05, 256, 256) as pl:
        args = (dD.ptr, (-6.4, -6.4), [(0.0, 0.0, 0.3)], [(4.0, 1.0)])
        cmd = pl.command(*args)[0]
        out = {"candidates": pl.K, "steps": p.steps, "command_per_call_ms": measure(lambda: pl.command(*args), calls, regions),
               "clearance_r20_plus_command_per_call_ms": measure(lambda: (plan.clearance(dG.ptr, 20, 0, 1, 256, 256, dD.ptr), pl.command(*args)), calls, regions),
               "chosen": [cmd.v, cmd.w, cmd.candidate, cmd.status]}
    dG.free(); dD.free()
    return out


def yardstick(calls, regions):
    W, H, B = 1280, 720, 32
    sp, cp = node.scan_params(W, H), costmap.costmap_params(from_cloud=1)
    maps, _ = formats_of(scene_q(sp, B, H, W, 7))
    fmt = subpix.I16_SUB
    poses = [(0.02 * k, 0.001 * k * k, 0.01 * k) for k in range(B)]
    bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
    hits = DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)
    dD = DeviceArray.from_numpy(maps[fmt])
    fp = subpix.subpix_params(fmt)
    out = {"size": [W, H], "batch": B,
           "subpix_costmap_i16_sub_per_call_ms": measure(lambda: subpix.subpix_costmap(sp, cp, fp, B, dD.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr), calls, regions)}
    with localmap.LocalMap(localmap.localmap_params(fmt), max_batch=B) as m:
        out["localmap_update_i16_sub_per_call_ms"] = measure(lambda: m.update(sp, poses, dD.ptr, W, H), calls, regions)
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    regions = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    L = jn.load()
    print(json.dumps({
        "script": "scripts/plan_rate.py", "timer": "HIP events" if HAVE_EVENTS else "host clock", "calls_per_region": calls, "regions": regions,
        "kernel_form": "k_clearance: one form (bit-packed halo in LDS, 8-row bands)",
        "clearance": clearance_rates(calls, regions), "plan": plan_rate(calls, regions), "yardstick": yardstick(calls, regions),
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

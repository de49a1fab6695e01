"""What the cost-to-go field (include/jn_route.h) costs next to the clearance field and the map update that feed it:
    python3 scripts/route_rate.py [calls_per_region] [regions]
The synchronous jn_route_field on one 256 x 256 map (the local map's default window: the whole form, one launch) and one 512 x 512 map
(the tiled form), each on an open map (a single obstacle cell), a cluttered random map (1 % obstacle cells and a few blocks of unknown
cells: plan_rate.py's grids; clearance radius 20, the default plan and route parameters) and the serpentine of tests/test_gpu_route.py
(corridors one cell wide, r2 = 0, no penalty), with the rounds and launches each took (jn_route_stats) and the share of cells reached;
jn_route_command for the default 33 candidates on the cluttered default map; and, in the same process with the same timer, jn_clearance
at radius 20 and jn_localmap_update on plan_rate.py's 1280x720 batch-32 workload as the yardsticks.  HIP events over regions of
`calls_per_region` calls after a warm-up, the median of `regions` regions, their minimum and maximum next to it.  Every call ends in a
synchronisation, so a region holds the launch and wait overhead of its calls as well as the kernels: `per_call_ms` is what a caller
pays.  Prints one JSON line."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import plan, route  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402
from plan_rate import grids, yardstick  # noqa: E402
from subpix_rate import HAVE_EVENTS, region_ms  # noqa: E402


def measure(fn, calls, regions):
    for _ in range(5):
        fn()
    ms = [region_ms(fn, calls) for _ in range(regions)]
    return {"per_call_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def serpentine(cy, cx):
    g = np.zeros((cy, cx), np.int8)
    g[1::2, :] = 100
    for k, row in enumerate(range(1, cy, 2)):
        g[row, cx - 1 if k % 2 == 0 else 0] = 0
    return g


def field_rates(side, calls, regions):
    pp = plan.plan_params()
    r2 = route.r2_of(pp, 0.05)
    open_map = np.zeros((side, side), np.int8)
    open_map[0, 0] = 100
    scenes = (("open", open_map, r2, route.route_params(), (side // 2, side // 2)),
              ("cluttered", grids(1, side, side, 3)[0], r2, route.route_params(), (side // 2, side // 2)),
              ("serpentine", serpentine(side, side), 0, route.route_params(near_radius=0, near_penalty=0, goal_radius=0), (0, 0)))
    out = {"grid": [1, side, side]}
    for name, grid, rr, rp, goal in scenes:
        dG = DeviceArray.from_numpy(grid); dD = DeviceArray((side, side), np.uint16); dT = DeviceArray((side, side), np.uint16)
        plan.clearance(dG.ptr, 20, 0, 1, side, side, dD.ptr)
        seeds, st = route.costtogo(dD.ptr, rr, rp, [goal], 1, side, side, dT.ptr, with_stats=True)
        row = measure(lambda: route.costtogo(dD.ptr, rr, rp, [goal], 1, side, side, dT.ptr), calls, regions)
        row.update({"form": "whole" if st.form == route.FORM_WHOLE else "tiled", "launches": st.launches, "rounds": st.rounds, "seeds": int(seeds[0]),
                    "reached_share": round(float((dT.numpy() != route.UNREACHED).mean()), 4)})
        if name == "cluttered":
            out["clearance_r20"] = measure(lambda: plan.clearance(dG.ptr, 20, 0, 1, side, side, dD.ptr), calls, regions)
            if side == 256:
                with plan.Plan(pp, 0.05, side, side) as pl:
                    rt = route.Route(pl)
                    args = (dD.ptr, dT.ptr, (-6.4, -6.4), [(0.0, 0.0, 0.3)])
                    cmd = rt.command(*args)[0]
                    out["route_command"] = measure(lambda: rt.command(*args), calls, regions)
                    out["route_command"].update({"candidates": pl.K, "steps": pp.steps, "chosen": [cmd.v, cmd.w, cmd.candidate, cmd.status]})
                    out["plan_command"] = measure(lambda: pl.command(dD.ptr, (-6.4, -6.4), [(0.0, 0.0, 0.3)], [(4.0, 1.0)]), calls, regions)
        out[name] = row
        dG.free(); dD.free(); dT.free()
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    regions = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    L = jn.load()
    print(json.dumps({
        "script": "scripts/route_rate.py", "timer": "HIP events" if HAVE_EVENTS else "host clock", "calls_per_region": calls, "regions": regions,
        "kernel_forms": "whole: k_route_relax<true>, one launch, the grid in one workgroup's LDS; tiled: k_route_init, batches of k_route_relax<false> over 256 x 256 tiles, k_route_final",
        "field": [field_rates(256, calls, regions), field_rates(512, calls, regions)], "yardstick": yardstick(calls, regions),
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

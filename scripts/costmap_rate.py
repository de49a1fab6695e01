"""What the obstacle costmap (include/jn_costmap.h) costs as the tail of the flagship workload, on one GPU:
    python3 scripts/costmap_rate.py [steps] [repeats]
ELAS 1280x720 D=128, batch 32, four slots, through jn_elas_submit_scan in bench.py's loop shape (a distinct input batch per slot, a
slot waited for before it is handed its next batch), timed WITHOUT and WITH the default costmap attached to every slot, the two
alternating `repeats` times in one process (A B A B ...: drift hits both alike); and the synchronous jn_obstacle_costmap (clear +
accumulate + finish of one batch of 32 maps) alone on the maps the last batch left.  Prints one JSON line.  The per-kernel times come from
running this script under `rocprofv3 --kernel-trace --stats`."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import costmap, node  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402

W, H, D, B, S, SCENE = 1280, 720, 128, 32, 4, 96


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    L = jn.load()
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    host_threads = 16 if ncpu >= 16 else max(2, ncpu - 1)
    Ls = np.empty((B, H, W), np.uint8); Rs = np.empty((B, H, W), np.uint8)
    for b in range(B):
        Ls[b], Rs[b] = node.synth_pair(W, H, SCENE, 12345 + b)
    rot = [(s * max(1, B // S)) % B for s in range(S)]
    dLs = [DeviceArray.from_numpy(np.roll(Ls, -rot[s], axis=0)) for s in range(S)]
    dRs = [DeviceArray.from_numpy(np.roll(Rs, -rot[s], axis=0)) for s in range(S)]
    bufs = [dict(d1=DeviceArray.from_numpy(np.zeros((B, H, W), np.float32)), d2=DeviceArray.from_numpy(np.zeros((B, H, W), np.float32)),
                 u8=DeviceArray((B, H, W), np.uint8), bins=DeviceArray((B, 90), np.float64), meta=DeviceArray((B, 4), np.float64),
                 st=(C.c_int32 * B)()) for _ in range(S)]
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    cp = costmap.costmap_params()
    grids = [(DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16), DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)) for _ in range(S)]
    p = jn.Elas.parameters(jn.Elas.ROBOTICS, disp_max=D - 1)
    with jn.Elas(p, W, H, max_batch=B, host_threads=host_threads, slots=S) as e:
        def run(k):
            inflight = []
            for i in range(k):
                slot = i % S
                if len(inflight) == S:
                    e.wait(inflight.pop(0))
                b = bufs[slot]
                e.submit_scan(slot, B, dLs[slot].ptr, dRs[slot].ptr, W, H * W, b["d1"].ptr, b["d2"].ptr, sp, lut.ptr, b["u8"].ptr, b["bins"].ptr,
                              b["meta"].ptr, b["st"])
                inflight.append(slot)
            while inflight:
                e.wait(inflight.pop(0))

        def attach(on):
            for s in range(S):
                costmap.attach(e, s, cp if on else None, grids[s][0].ptr, grids[s][1].ptr)

        def timed():
            L.jn_device_synchronize(0)
            t0 = time.perf_counter()
            run(steps)
            L.jn_device_synchronize(0)
            return steps * B / (time.perf_counter() - t0)

        run(3 * S)                                               # warm-up: allocations, clocks, the slots' pipelines
        attach(True); run(S); attach(False)
        plain, attached = [], []
        for _ in range(repeats):
            attach(False); plain.append(timed())
            attach(True); attached.append(timed())
        # the synchronous call alone, on the u8 maps / bins slot 0's last batch left
        hits, grid = grids[0]
        for _ in range(5):
            costmap.obstacle_costmap(sp, cp, B, bufs[0]["u8"].ptr, lut.ptr, W, H, bufs[0]["bins"].ptr, hits.ptr, grid.ptr)
        t0 = time.perf_counter()
        reps = 50
        for _ in range(reps):
            costmap.obstacle_costmap(sp, cp, B, bufs[0]["u8"].ptr, lut.ptr, W, H, bufs[0]["bins"].ptr, hits.ptr, grid.ptr)
        call_ms = (time.perf_counter() - t0) / reps * 1e3
        g = grid.numpy()
        attach(False)
    mp, ma = statistics.median(plain), statistics.median(attached)
    print(json.dumps({
        "script": "scripts/costmap_rate.py", "workload": "ELAS %dx%d D=%d batch %d, %d slots, jn_elas_submit_scan; default costmap (128x128 cells of 0.05 m)" % (W, H, D, B, S),
        "steps_per_region": steps, "regions_each": repeats, "host_threads": host_threads,
        "pairs_per_s_plain": [round(x, 1) for x in plain], "pairs_per_s_attached": [round(x, 1) for x in attached],
        "pairs_per_s_plain_median": round(mp, 1), "pairs_per_s_attached_median": round(ma, 1),
        "attached_cost_percent": round(100.0 * (mp - ma) / mp, 2),
        "plain_spread_percent": round(100.0 * (max(plain) - min(plain)) / mp, 2),
        "standalone_call_ms_per_batch": round(call_ms, 4),
        "cells_occupied_free_unknown_frame0": [int((g[0] == 100).sum()), int((g[0] == 0).sum()), int((g[0] == -1).sum())],
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

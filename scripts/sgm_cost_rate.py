"""What the SGM mode costs over a cost volume (include/jn_sgm_cost.h), next to the plain mode in the same process:
    python3 scripts/sgm_cost_rate.py [batches_per_leg] [out.json] [census]
1280x720 D = 128 batch 32, four slots in flight (jn_sgm_submit_scan without scan parameters), plain handle and BLOCK_SSD handle
alternating; then producer and sweeps separately (jn_sgm_cost_volume, jn_sgm_aggregate_batch: synchronous calls, stage times from
jn_sgm_last_times).  The same at BASELINE.json config 5's share: 1920x1080 D = 256 sub-pixel batch 8.
With `census` a third leg joins the alternation: a CENSUS handle (9x7 window, cost_max = 62), with its producer and sweeps separately.
Refuses to run without a GPU.  Prints one JSON line (and writes it to out.json when given)."""
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import sgm  # noqa: E402
from jackal_navigation_amd.device import DeviceArray, device_count  # noqa: E402
import scenes  # noqa: E402


def pairs_of(W, H, B, D, distinct=4):
    kinds = ("strips", "blobs", "periodic", "blobs")
    ps = [scenes.make_scene(kinds[t % 4], W, H, min(100, D - 28), 40 + t) for t in range(distinct)]
    L = np.stack([ps[t % distinct][0] for t in range(B)]); R = np.stack([ps[t % distinct][1] for t in range(B)])
    return DeviceArray.from_numpy(L), DeviceArray.from_numpy(R)


def pipelined(m, B, S, dL, dR, W, H, dd, batches):
    def sub(s):
        m.submit_scan(s, B, dL.ptr, dR.ptr, W, H * W, dd[s].ptr)
    for s in range(S):
        sub(s)
    t0 = time.perf_counter()
    for k in range(batches):
        m.wait(k % S); sub(k % S)
    dt = time.perf_counter() - t0
    for s in range(S):
        m.wait(s)
    return round(batches * B / dt, 1)


def config(W, H, D, B, S, sub, batches, census=False):
    out = {"size": [W, H], "D": D, "batch": B, "slots": S, "subpixel": sub, "batches_per_leg": batches}
    dL, dR = pairs_of(W, H, B, D)
    dd = [DeviceArray((B, H, W), np.int16) for _ in range(S)]
    p = jn.Sgm.parameters(num_disparities=D, subpixel=sub)
    c = jn.Sgm.cost_parameters()
    out["cost"] = {k: getattr(c, k) for k, _ in c._fields_}
    handles = contextlib.ExitStack()
    with handles:
        plain = handles.enter_context(jn.Sgm(p, W, H, max_batch=B)); blk = handles.enter_context(jn.Sgm(p, W, H, max_batch=B, cost=c))
        named = [("plain", plain), ("block_ssd", blk)]
        if census:
            cc = jn.Sgm.cost_parameters(cost_function=sgm.SGM_COST_CENSUS, block_radius=4, cost_max=62)
            out["census_cost"] = {k: getattr(cc, k) for k, _ in cc._fields_}
            cen = handles.enter_context(jn.Sgm(p, W, H, max_batch=B, cost=cc))
            named.append(("census", cen))
        legs = {name: [] for name, _ in named}
        for _, m in named:
            pipelined(m, B, S, dL, dR, W, H, dd, S)               # warm-up: every slot allocates
        for _ in range(3):
            for name, m in named:
                legs[name].append(pipelined(m, B, S, dL, dR, W, H, dd, batches))
        for name, _ in named:
            out[name + "_pairs_per_s"] = legs[name]
        out["valid_fraction"] = {}
        for name, m in named:
            m.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd[0].ptr)
            out["valid_fraction"][name] = round(float((dd[0].numpy() >= 0).mean()), 4)
        # the stages of a lone synchronous batch
        for name, m in named:
            ts = []
            for _ in range(5):
                m.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd[0].ptr)
                ts.append(m.last_times())
            out[name + "_lone_batch_ms"] = {k: round(statistics.median(t[k] for t in ts), 3) for k in ts[0]}
        # producer and sweeps on their own
        dC = DeviceArray((B, H, W, D), np.uint8)
        tp, ta = [], []
        for _ in range(5):
            t0 = time.perf_counter(); blk.cost_volume(B, dL.ptr, dR.ptr, W, H * W, dC.ptr); tp.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); blk.aggregate(B, dC.ptr, dd[0].ptr); ta.append((time.perf_counter() - t0) * 1e3)
        out["producer_call_ms"] = round(statistics.median(tp), 3)
        out["aggregate_call_ms"] = round(statistics.median(ta), 3)
        out["producer_GBps_written"] = round(B * W * H * D / (statistics.median(tp) * 1e-3) / 1e9, 1)
        if census:
            tp, ta = [], []
            for _ in range(5):
                t0 = time.perf_counter(); cen.cost_volume(B, dL.ptr, dR.ptr, W, H * W, dC.ptr); tp.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); cen.aggregate(B, dC.ptr, dd[0].ptr); ta.append((time.perf_counter() - t0) * 1e3)
            out["census_producer_call_ms"] = round(statistics.median(tp), 3)
            out["census_aggregate_call_ms"] = round(statistics.median(ta), 3)
            out["census_producer_GBps_written"] = round(B * W * H * D / (statistics.median(tp) * 1e-3) / 1e9, 1)
        dC.free()
    for a in [dL, dR] + dd:
        a.free()
    return out


def main():
    if device_count() < 1:
        sys.exit("sgm_cost_rate.py needs a GPU")
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    census = "census" in sys.argv[3:]
    what = "SGM over a block-SSD cost volume vs the plain mode" + (" vs a census cost volume" if census else "")
    res = {"what": what, "hd720": config(1280, 720, 128, 32, 4, 0, batches, census),
           "config5_share": config(1920, 1080, 256, 8, 4, 1, batches, census)}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

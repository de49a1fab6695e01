"""What the SGM mode costs over a block-SSD cost volume (include/jn_sgm_cost.h), next to the plain mode in the same process:
    python3 scripts/sgm_cost_rate.py [batches_per_leg] [out.json]
1280x720 D = 128 batch 32, four slots in flight (jn_sgm_submit_scan without scan parameters), plain handle and BLOCK_SSD handle
alternating; then producer and sweeps separately (jn_sgm_cost_volume, jn_sgm_aggregate_batch: synchronous calls, stage times from
jn_sgm_last_times).  The same at BASELINE.json config 5's share: 1920x1080 D = 256 sub-pixel batch 8.
Refuses to run without a GPU.  Prints one JSON line (and writes it to out.json when given)."""
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


def config(W, H, D, B, S, sub, batches):
    out = {"size": [W, H], "D": D, "batch": B, "slots": S, "subpixel": sub, "batches_per_leg": batches}
    dL, dR = pairs_of(W, H, B, D)
    dd = [DeviceArray((B, H, W), np.int16) for _ in range(S)]
    p = jn.Sgm.parameters(num_disparities=D, subpixel=sub)
    c = jn.Sgm.cost_parameters()
    out["cost"] = {k: getattr(c, k) for k, _ in c._fields_}
    with jn.Sgm(p, W, H, max_batch=B) as plain, jn.Sgm(p, W, H, max_batch=B, cost=c) as blk:
        legs = {"plain": [], "block_ssd": []}
        for m in (plain, blk):
            pipelined(m, B, S, dL, dR, W, H, dd, S)               # warm-up: every slot allocates
        for _ in range(3):
            legs["plain"].append(pipelined(plain, B, S, dL, dR, W, H, dd, batches))
            legs["block_ssd"].append(pipelined(blk, B, S, dL, dR, W, H, dd, batches))
        out["plain_pairs_per_s"] = legs["plain"]; out["block_ssd_pairs_per_s"] = legs["block_ssd"]
        out["valid_fraction"] = {}
        for name, m in (("plain", plain), ("block_ssd", blk)):
            m.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd[0].ptr)
            out["valid_fraction"][name] = round(float((dd[0].numpy() >= 0).mean()), 4)
        # the stages of a lone synchronous batch
        for name, m in (("plain", plain), ("block_ssd", blk)):
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
        dC.free()
    for a in [dL, dR] + dd:
        a.free()
    return out


def main():
    if device_count() < 1:
        sys.exit("sgm_cost_rate.py needs a GPU")
    batches = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    res = {"what": "SGM over a block-SSD cost volume vs the plain mode", "hd720": config(1280, 720, 128, 32, 4, 0, batches),
           "config5_share": config(1920, 1080, 256, 8, 4, 1, batches)}
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""What the disparity post-filter (include/jn_postfilter.h) costs:
    python3 scripts/postfilter_rate.py [calls_per_region] [regions]
Synchronous call: jn_disparity_postfilter in place at 1280x720 batch 32 and 1920x1080 batch 8, both int16 formats, on real SGM output
(tests/scenes.py kinds strips / blobs / periodic, four pairs repeated through the batch) and on the worst cases of the labelling (a
one-pixel spiral through the frame, a checkerboard of valid / invalid pixels, one segment covering the frame), median off and on, timed
by HIP events over regions of `calls_per_region` calls after a warm-up (the input is uploaded again before every region: the filter
works in place).  Every call ends in a stream synchronisation, so `per_call_ms` is what a caller pays.
Attached: SGM pairs/s at 1280x720 batch 32, D = 128, six slots in flight with scan parameters — nothing attached (the one-kernel tail),
the filter attached to every slot (which queues the three-kernel tail), alternating in the same process; the three-kernel tail alone is
measured by the hooks build's A/B switch in a separate process (scripts/sgm_round.sh), not here.
Block matching: SSD, four slots, 1280x720 batch 32, without scan parameters, then the recipe of the header per batch: the filter in
place, jn_sgm_disparity_to_u8, jn_obstacle_scan (all synchronous).
Refuses to run without a GPU.  Prints one JSON line."""
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
from jackal_navigation_amd import node, postfilter  # noqa: E402
from jackal_navigation_amd.device import DeviceArray, device_count  # noqa: E402
import scenes  # noqa: E402
from postfilter_def import spiral  # noqa: E402

try:
    import torch
    HAVE_EVENTS = torch.cuda.is_available()
except Exception:  # pragma: no cover
    HAVE_EVENTS = False


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


def pairs_of(W, H, B, distinct=4):
    kinds = ("strips", "blobs", "periodic", "blobs")
    ps = [scenes.make_scene(kinds[t % 4], W, H, 100, 40 + t) for t in range(distinct)]
    L = np.stack([ps[t % distinct][0] for t in range(B)]); R = np.stack([ps[t % distinct][1] for t in range(B)])
    return DeviceArray.from_numpy(L), DeviceArray.from_numpy(R)


def sync_rates(W, H, B, calls, regions):
    out = {"size": [W, H], "batch": B}
    dL, dR = pairs_of(W, H, B)
    cases = {}
    for sub in (0, 1):
        dd = DeviceArray((B, H, W), np.int16)
        with jn.Sgm(jn.Sgm.parameters(num_disparities=128, subpixel=sub), W, H, max_batch=B) as m:
            m.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd.ptr)
        cases["sgm_" + ("i16_sub" if sub else "i16")] = (postfilter.I16_SUB if sub else postfilter.I16, dd.numpy())
        dd.free()
    yy, xx = np.mgrid[0:H, 0:W]
    for name, m in (("spiral", spiral(H, W)), ("checkerboard", np.where((yy + xx) % 2 == 0, 30, -1).astype(np.int16)),
                    ("one_segment", np.full((H, W), 40, np.int16))):
        cases[name + "_i16"] = (postfilter.I16, np.broadcast_to(m, (B, H, W)).copy())
    st = DeviceArray((B, 4), np.uint32)
    for name, (fmt, maps) in cases.items():
        d = DeviceArray.from_numpy(maps)
        for median in (0, 1):
            fp = postfilter.postfilter_params(fmt, median=median)

            def region():
                d.upload(maps)
                return region_ms(lambda: postfilter.disparity_postfilter(fp, B, d.ptr, W, H, None, st.ptr), calls)
            region()
            # the first call of a region filters the raw map, the others its own output (fewer speckles, the same segments)
            d.upload(maps)
            first = region_ms(lambda: postfilter.disparity_postfilter(fp, B, d.ptr, W, H, None, st.ptr), 1)
            stats = st.numpy().astype(np.int64).sum(axis=0).tolist()
            key = "%s%s" % (name, "_median" if median else "")
            out[key + "_per_call_ms"] = round(statistics.median(region() for _ in range(regions)), 4)
            out[key + "_first_call_ms"] = round(first, 4)
            out[key + "_stats"] = stats
        d.free()
    dL.free(); dR.free(); st.free()
    return out


def sgm_slots(calls):
    W, H, B, S = 1280, 720, 32, 6
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    dL, dR = pairs_of(W, H, B)
    bufs = [dict(dd=DeviceArray((B, H, W), np.int16), u8=DeviceArray((B, H, W), np.uint8), bins=DeviceArray((B, sp.bins), np.float64),
                 meta=DeviceArray((B, 4), np.float64), st=DeviceArray((B, 4), np.uint32)) for _ in range(S)]
    out = {"size": [W, H], "batch": B, "slots": S, "batches_per_leg": calls * S, "detached_pairs_per_s": [], "attached_pairs_per_s": []}
    fp = postfilter.postfilter_params(postfilter.I16)
    with jn.Sgm(jn.Sgm.parameters(num_disparities=128), W, H, max_batch=B) as m:
        def leg():
            def sub(s):
                b = bufs[s]
                m.submit_scan(s, B, dL.ptr, dR.ptr, W, H * W, b["dd"].ptr, sp, lut.ptr, b["u8"].ptr, b["bins"].ptr, b["meta"].ptr)
            for s in range(S):
                sub(s)
            t0 = time.perf_counter()
            for k in range(calls * S):
                m.wait(k % S); sub(k % S)
            dt = time.perf_counter() - t0
            for s in range(S):
                m.wait(s)
            return round(calls * S * B / dt, 1)
        leg()
        for rep in range(3):
            out["detached_pairs_per_s"].append(leg())
            for s in range(S):
                m.attach_postfilter(s, fp, bufs[s]["st"].ptr)
            if rep == 0:
                leg()
            out["attached_pairs_per_s"].append(leg())
            for s in range(S):
                m.attach_postfilter(s)
        out["removed_pixels_last_batch"] = int(bufs[0]["st"].numpy()[:, 3].sum())
    out["detached_median"] = statistics.median(out["detached_pairs_per_s"]); out["attached_median"] = statistics.median(out["attached_pairs_per_s"])
    return out


def bm_recipe(calls):
    from jackal_navigation_amd.bm import COST_SSD
    W, H, B, S = 1280, 720, 32, 4
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    dL, dR = pairs_of(W, H, B)
    bufs = [dict(dd=DeviceArray((B, H, W), np.int16), st=DeviceArray((B, 4), np.uint32)) for _ in range(S)]
    u8 = DeviceArray((B, H, W), np.uint8); bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
    fp = postfilter.postfilter_params(postfilter.I16)
    out = {"size": [W, H], "batch": B, "slots": S, "batches_per_leg": calls * S}
    with jn.Bm(jn.Bm.parameters(num_disparities=128, cost_function=COST_SSD), W, H, max_batch=B) as m:
        def leg(mode):
            for s in range(S):
                m.submit_scan(s, B, dL.ptr, dR.ptr, W, H * W, bufs[s]["dd"].ptr)
            t0 = time.perf_counter()
            for k in range(calls * S):
                s = k % S
                m.wait(s)
                if mode >= 1:
                    postfilter.disparity_postfilter(fp, B, bufs[s]["dd"].ptr, W, H, None, bufs[s]["st"].ptr)
                if mode >= 2:
                    m.to_u8(bufs[s]["dd"].ptr, u8.ptr, B * W * H)
                    node.obstacle_scan(sp, B, u8.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
                m.submit_scan(s, B, dL.ptr, dR.ptr, W, H * W, bufs[s]["dd"].ptr)
            dt = time.perf_counter() - t0
            for s in range(S):
                m.wait(s)
            return round(calls * S * B / dt, 1)
        leg(2)
        for name, mode in (("matcher_only", 0), ("plus_filter", 1), ("plus_filter_u8_scan", 2)):
            out[name + "_pairs_per_s"] = statistics.median(leg(mode) for _ in range(3))
        out["removed_pixels_last_batch"] = int(bufs[0]["st"].numpy()[:, 3].sum())
    return out


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    regions = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    if device_count() < 1:
        sys.exit("scripts/postfilter_rate.py needs a GPU")
    L = jn.load()
    print(json.dumps({
        "script": "scripts/postfilter_rate.py", "timer": "HIP events" if HAVE_EVENTS else "host clock", "calls_per_region": calls, "regions": regions,
        "synchronous": [sync_rates(1280, 720, 32, calls, regions), sync_rates(1920, 1080, 8, calls, regions)],
        "sgm_six_slots": sgm_slots(max(4, calls // 4)),
        "bm_ssd_four_slots": bm_recipe(max(4, calls // 4)),
        "version": L.jn_version().decode(),
    }))


if __name__ == "__main__":
    main()

"""What the ground-plane estimator (include/jn_ground.h) costs on one GPU:
    python3 scripts/ground_rate.py [repeats] [calls_per_region] [--trace DIR]
jn_ground_estimate on a batch of 32 maps at 1280x720 (the default region: the lower half), for K = 64 / 256 / 1024 hypotheses and the three
input formats.  The maps are a rendered floor of the default rig with +-0.3 px noise, a wall across the top of the region and 10 %
invalid pixels.  Per configuration: warm-up calls, then `repeats` timed regions of `calls_per_region` synchronous calls each (a host clock
around calls that end in a stream synchronise; the call includes the clears, the four kernels, the copies back and the host solve); the
median region is reported, with the spread.  Prints one JSON line.
--trace DIR: afterwards ONE run of the default configuration per format under `rocprofv3 --kernel-trace --stats` (a fresh child process, the
program after `--`, under its own time limit; not started when the timed part failed) and the per-kernel summary from its stats file
goes into the line as "kernels" (average ns per launch = per batch of 32)."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import ground, node  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402

W, H, B = 1280, 720, 32
FORMATS = (("f32", ground.F32), ("i16", ground.I16), ("i16_sub", ground.I16_SUB))


def floor_maps(sp):
    """[B][H][W] float64 disparities: the robot-frame plane z = 0 seen by the default rig, noise, a wall, holes; -10 where invalid."""
    rng = np.random.default_rng(2026)
    XR, XT = np.array(sp.XR).reshape(3, 3), np.array(sp.XT)
    Q = np.array(sp.Q).reshape(4, 4)
    pd = Q.T @ np.array([XR[2, 0], XR[2, 1], XR[2, 2], XT[2]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    d = -(pd[0] * xs + pd[1] * ys + pd[3]) / pd[2]
    maps = np.empty((B, H, W), np.float64)
    for b in range(B):
        m = d + rng.uniform(-0.3, 0.3, (H, W))
        m[H // 2:H // 2 + 40] = 30.0 + rng.uniform(-0.3, 0.3, (40, W))
        m[(d < 1.0) | (rng.random((H, W)) < 0.10)] = -10.0
        maps[b] = m
    return maps


def as_format(maps, fmt):
    if fmt == ground.F32:
        return maps.astype(np.float32)
    if fmt == ground.I16:
        return np.where(maps < 0, -1, np.rint(maps)).astype(np.int16)
    return np.where(maps < 0, -16, np.rint(16 * maps)).astype(np.int16)


def child(calls):
    """The traced program: the default configuration, each format, `calls` calls."""
    sp = node.scan_params(W, H)
    maps = floor_maps(sp)
    gp = ground.ground_params(W, H)
    for name, fmt in FORMATS:
        d = DeviceArray.from_numpy(as_format(maps, fmt))
        for _ in range(calls):
            ground.estimate(sp, gp, B, d.ptr, fmt, W, H)
        d.free()


def kernel_summary(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return None
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r["Name"].replace("jnav::(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        rows.append({"kernel": name, "calls": int(r["Calls"]), "average_ns": round(float(r["AverageNs"]), 1), "min_ns": int(float(r["MinNs"])),
                     "max_ns": int(float(r["MaxNs"])), "percent": float(r["Percentage"])})
    return rows


def main():
    args = [a for a in sys.argv[1:]]
    if args and args[0] == "--child":
        return child(int(args[1]))
    trace = None
    if "--trace" in args:
        i = args.index("--trace")
        trace = args[i + 1]
        del args[i:i + 2]
    repeats = int(args[0]) if len(args) > 0 else 7
    calls = int(args[1]) if len(args) > 1 else 20
    L = jn.load()
    sp = node.scan_params(W, H)
    maps = floor_maps(sp)
    region_pixels = (H - H // 2) * W
    results, example = [], None
    for name, fmt in FORMATS:
        d = DeviceArray.from_numpy(as_format(maps, fmt))
        for K in (64, 256, 1024):
            gp = ground.ground_params(W, H, hypotheses=K)
            for _ in range(3):                                   # warm-up: code objects, the scratch allocation, clocks
                planes = ground.estimate(sp, gp, B, d.ptr, fmt, W, H)
            times = []
            for _ in range(repeats):
                L.jn_device_synchronize(0)
                t0 = time.perf_counter()
                for _ in range(calls):
                    planes = ground.estimate(sp, gp, B, d.ptr, fmt, W, H)
                times.append((time.perf_counter() - t0) / calls * 1e3)
            med = statistics.median(times)
            results.append({"format": name, "hypotheses": K, "ms_per_batch_median": round(med, 4), "ms_per_batch_min": round(min(times), 4),
                            "ms_per_batch_max": round(max(times), 4), "us_per_map": round(med / B * 1e3, 2),
                            "plane_evaluations_per_batch": B * region_pixels * K,
                            "g_evaluations_per_s": round(B * region_pixels * K / (med * 1e-3) / 1e9, 1),
                            "frames_ok": sum(1 for p in planes if p.status == 0)})
            if K == 256 and fmt == ground.F32:
                XR, XT, tilt = ground.extrinsics(planes, sp)
                p = planes[0]
                example = {"inlier_share_frame0": round(p.inliers / max(1, p.valid), 4), "rms_px_frame0": round(p.rms, 4),
                           "height_m_joint": round(float(XT[2]), 5), "tilt_from_the_true_rig_deg": round(tilt, 4)}
        d.free()
    line = {"script": "scripts/ground_rate.py", "workload": "jn_ground_estimate, %d maps of %dx%d, region = lower half (%d pixels a map)" % (B, W, H, region_pixels),
            "regions_each": repeats, "calls_per_region": calls, "results": results, "example_f32_k256": example, "version": L.jn_version().decode()}
    if trace:
        os.makedirs(trace, exist_ok=True)
        cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace, "--",
               sys.executable, os.path.abspath(__file__), "--child", "10"]
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL).returncode
        line["trace_rc"] = rc
        if rc == 0:
            s = kernel_summary(trace)
            if s:
                line["kernels"] = [r for r in s if "k_ground" in r["kernel"]]
    print(json.dumps(line))


if __name__ == "__main__":
    main()

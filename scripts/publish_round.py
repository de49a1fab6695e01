#!/usr/bin/env python3
"""Copy the evidence set scripts/round6_profiles.sh <tag> left under gpurun_out/ into profiles/ (tracked) and write
profiles/<tag>_manifest.json: every published file, the sha256 of the kernel sources it was measured on, the commit.
    python3 scripts/publish_round.py <tag>
Files are taken NEWEST FIRST (gpurun_out/ accumulates merged results of several calls; round 2 published stale ones)."""
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

tag = sys.argv[1]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
g, p = os.path.join(root, "gpurun_out"), os.path.join(root, "profiles")
rnd = tag.split("_")[0]


def newest(pattern):
    files = sorted(glob.glob(os.path.join(g, pattern)), key=os.path.getmtime)
    return files[-1] if files else None


def sha(rel):
    return hashlib.sha256(open(os.path.join(root, rel), "rb").read()).hexdigest()


published = {}

# A refresh with nothing new is a no-op (VERDICT r03 #7d): the manifest remembers the newest modification time among the inputs it
# was made from; if no gpurun_out/<tag>_* file is newer, nothing is rewritten (git then sees no change at all).
_inputs = [f for f in glob.glob(os.path.join(g, "%s_*" % tag)) + glob.glob(os.path.join(g, "%s_*/*/*" % tag)) if os.path.isfile(f)]
_newest_in = max([os.path.getmtime(f) for f in _inputs], default=0.0)
try:
    _old = json.load(open(os.path.join(p, "%s_manifest.json" % tag)))
    if _inputs and _old.get("inputs_newest_mtime") == _newest_in and "--force" not in sys.argv:
        print("profiles/%s_*: nothing new under gpurun_out/ since the manifest was written: no-op" % tag)
        sys.exit(0)
except (OSError, ValueError):
    pass


def put(src, name):
    if src and os.path.exists(src) and os.path.getsize(src) > 0:
        shutil.copyfile(src, os.path.join(p, name))
        published[name] = os.path.relpath(src, root)


put(newest("%s_slots1/*/*kernel_stats.csv" % tag), "%s_slots1_kernel_stats.csv" % tag)
put(newest("%s_default/*/*kernel_stats.csv" % tag), "%s_default_bench_kernel_stats.csv" % tag)
put(newest("%s_sgm/*/*kernel_stats.csv" % tag), "%s_sgm_kernel_stats.csv" % tag)
put(newest("%s_bm/*/*kernel_stats.csv" % tag), "%s_bm_kernel_stats.csv" % tag)
put(newest("%s_bm_ssd/*/*kernel_stats.csv" % tag), "%s_bm_ssd_kernel_stats.csv" % tag)
for src, name in (("default_bench_line.json", "default_bench_line_under_rocprof.json"), ("default_occupancy.txt", "default_bench_occupancy.txt"),
                  ("pmc_FETCH_SIZE.txt", None), ("pmc_WRITE_SIZE.txt", None), ("bench_line.json", None), ("sgm_bench_line.json", None),
                  ("sgm_pmc_FETCH_SIZE.txt", None), ("sgm_pmc_WRITE_SIZE.txt", None), ("sgm_pmc_SQ.txt", None),
                  ("sgm_strips_ab.txt", None), ("sgm_slots_ab.txt", None), ("bm_slots_ab.txt", None), ("bm_bench_line.json", None), ("bm_config2_bench_line.json", None), ("other_configs.jsonl", None),
                  ("merge_in_worker.txt", None), ("node_rate.txt", None), ("latency_check.txt", None), ("host_pointer_rate.txt", None),
                  ("valu_rate_probe.txt", None), ("stage_a_priority_ab.txt", None), ("pace_ab.txt", None), ("parity_sweep.txt", None), ("sgm_stress.txt", None),
                  ("bm_ssd_bench_line.json", None), ("bm_ssd_1080p_bench_line.json", None), ("bm_sad_1080p_bench_line.json", None), ("bm_ssd_pmc_mfma.txt", None),
                  ("host_threads.txt", None), ("pk3_probe.txt", None), ("dep_chain_probe.txt", None), ("lds_unaligned_probe.txt", None), ("op_rate_probe.txt", None),
                  ("dense_dbg_switches.txt", None), ("hw_queues_ab.txt", None), ("gate_ab.txt", None), ("lone_timeline.txt", None), ("gpu_tests.txt", None),
                  ("gpu_delaunay_ab.txt", None), ("lone_env_ab.txt", None), ("fetch_size_probe.txt", None), ("dt_no_volatile.txt", None),
                  ("slot_timeline.txt", None), ("full_hd_routes.txt", None), ("lone_wave_probe.txt", None), ("lds_misaligned_store_probe.txt", None),
                  ("matcher_kernel_coverage.txt", None), ("suite_kernel_coverage.txt", None)):
    put(os.path.join(g, "%s_%s" % (tag, src)), "%s_%s" % (tag, name or src))
for name, how in (("matcher_kernel_coverage.txt", "scripts/kernel_coverage.py --matchers on the kernel trace of tests/test_gpu_matcher_matrix.py tests/test_gpu_sgm.py tests/test_gpu_bm.py"),
                  ("suite_kernel_coverage.txt", "scripts/kernel_coverage.py on the kernel trace of the whole -m gpu suite (bench tests excluded)")):
    if "%s_%s" % (tag, name) in published:
        published["%s_%s" % (tag, name)] = how                  # a listing derived from a trace: what made it
sq = "".join(open(f).read() for f in (os.path.join(g, "%s_sq1.txt" % tag), os.path.join(g, "%s_sq2.txt" % tag)) if os.path.exists(f))
if sq:
    open(os.path.join(p, "%s_pmc_SQ.txt" % tag), "w").write(sq)
    published["%s_pmc_SQ.txt" % tag] = "gpurun_out/%s_sq{1,2}.txt" % tag
for name in list(published):                      # bench lines: keep only the JSON line
    if name.endswith("bench_line.json") or name.endswith("under_rocprof.json"):
        lines = [l for l in open(os.path.join(p, name)) if l.startswith('{"metric"')]
        if lines:
            open(os.path.join(p, name), "w").write(lines[-1])
subprocess.run([sys.executable, os.path.join(root, "scripts", "make_pmc_json.py"), tag, os.path.join(p, "%s_pmc_traffic.json" % rnd)], check=True, stdout=subprocess.DEVNULL)
published["%s_pmc_traffic.json" % rnd] = "scripts/make_pmc_json.py %s" % tag


def counters(path):
    res, cur = {}, None
    for line in open(path):
        if not line.startswith(" "):
            cur = re.sub(r"^void ", "", line.strip()); res[cur] = {}
        else:
            f = line.split(); res[cur][f[0]] = float(f[1])
    return res


fs, ws = os.path.join(p, "%s_sgm_pmc_FETCH_SIZE.txt" % tag), os.path.join(p, "%s_sgm_pmc_WRITE_SIZE.txt" % tag)
if os.path.exists(fs) and os.path.exists(ws):     # SGM traffic from its own PMC passes
    f, w = counters(fs), counters(ws)
    ker = {}
    for k in sorted(set(f) | set(w)):
        ker[k] = {"FETCH_SIZE_KB": f.get(k, {}).get("FETCH_SIZE"), "WRITE_SIZE_KB": w.get(k, {}).get("WRITE_SIZE")}
        if None not in ker[k].values():
            ker[k]["traffic_bytes"] = int(2 * ker[k]["FETCH_SIZE_KB"] * 1024 + ker[k]["WRITE_SIZE_KB"] * 1024)
    total = sum(v.get("traffic_bytes", 0) for v in ker.values())
    json.dump({"command": "rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE (separate passes) -- python3 bench.py --mode sgm --steps 2 --warmup 1 --no-cpu-baseline",
               "workload": [1280, 720, 128, 32], "correction": "gfx950: FETCH_SIZE x 2 (MI355X_MICROARCH.md, HBM; measured: the counter shows half the bytes read for 4-, 8- and 16-byte-per-lane loads alike, profiles/%s_fetch_size_probe.txt); WRITE_SIZE as is; KB = 1024 B" % tag,
               "sgm_sweep_sha256": sha("jackal_navigation_amd/csrc/sgm_sweep.hip"), "kernels": ker, "bytes_per_batch": total,
               "algorithmic_bytes_per_batch": int((4 * 1280 * 720 * 128 + 5 * 1280 * 720) * 32)}, open(os.path.join(p, "%s_sgm_pmc_traffic.json" % rnd), "w"), indent=1)
    published["%s_sgm_pmc_traffic.json" % rnd] = "from %s_sgm_pmc_*.txt" % tag
manifest = {"tag": tag, "commit": subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip(),
            "sources_sha256": {f: sha(f) for f in ("jackal_navigation_amd/csrc/kernels.hip", "jackal_navigation_amd/csrc/scan.hip", "jackal_navigation_amd/csrc/sgm_sweep.hip", "jackal_navigation_amd/csrc/bm.hip", "jackal_navigation_amd/csrc/bm_mfma.hip", "jackal_navigation_amd/csrc/prefilter.h",
                                                   "jackal_navigation_amd/csrc/delaunay_gpu.hip", "jackal_navigation_amd/csrc/elas_api.cpp", "jackal_navigation_amd/csrc/elas_batch.cpp", "bench.py")},
            "inputs_newest_mtime": _newest_in, "files": published}
json.dump(manifest, open(os.path.join(p, "%s_manifest.json" % tag), "w"), indent=1)
open(os.path.join(p, "CURRENT"), "w").write(tag + "\n")
print("published %d files for %s" % (len(published), tag))

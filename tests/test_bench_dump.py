"""`bench.py --dump-outputs DIR`: what the last timed step handed its caller, as .npy files two builds can be compared by."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("jn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way_every_time(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, (24, 720, 1280), dtype=np.uint8)           # 88 MB as float32: over the budget on its own
    arrays = {"maps": big, "maps_f32": big.astype(np.float32) / 3, "bins": rng.random((24, 90)), "status": np.arange(24, dtype=np.int32)}
    rep = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert rep[0]["arrays"] == rep[1]["arrays"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in arrays) == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_MAX_BYTES < 64e6
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for name, g in got.items():
        assert g.dtype == (np.float64 if arrays[name].dtype == np.float64 else np.float32), name
        assert np.array_equal(g, np.load(tmp_path / "b" / (name + ".npy"))), name
    assert np.array_equal(got["bins"], arrays["bins"]) and np.array_equal(got["status"], arrays["status"])
    assert not rep[0]["arrays"]["bins"]["sampled"] and rep[0]["arrays"]["maps"]["sampled"] and rep[0]["arrays"]["maps_f32"]["sampled"]
    for name in ("maps", "maps_f32"):                                     # a sample is elements of the array, in the array's order
        k = got[name].size
        assert k > big.size // 8 and k == rep[0]["arrays"][name]["elements_written"]
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(big.size, size=k, replace=False))
        assert np.array_equal(got[name], arrays[name].reshape(-1)[idx].astype(np.float32)), name


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dumps_the_last_timed_step_and_steps_sets_the_timed_steps(tmp_path, oracle):
    """Three timed steps over two slots end on slot 0, whose batch is seeds 12345, 12346: the dumped arrays are that batch's answers
    (D1 / D2 / u8 map bit-identical to the oracle's, the scan within its tolerance), and the line says one region of three steps."""
    W, H, B, scene, D = 320, 180, 2, 48, 256
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(W), "--height", str(H), "--disp", str(D),
           "--scene-disp", str(scene), "--batch", str(B), "--slots", "2", "--min-time", "0", "--no-cpu-baseline", "--no-latency-config", "--dump-outputs", str(tmp_path / "out")]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    j = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 3 and j["timing"]["regions"] == 1 and j["config"]["pairs_failed"] == 0
    assert j["dump_outputs"]["dir"] == str(tmp_path / "out") and not any(v["sampled"] for v in j["dump_outputs"]["arrays"].values())
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(got) == ["D1", "D2", "disparity_u8", "scan_bins", "scan_meta"]
    assert all(g.dtype in (np.float32, np.float64) for g in got.values())
    assert got["D1"].shape == got["D2"].shape == got["disparity_u8"].shape == (B, H, W) and got["scan_bins"].shape == (B, 90)
    assert all(np.isfinite(g).all() and np.any(g != 0) for g in got.values())                      # computed arrays, none left as allocated
    spo = oracle.scan_params(W, H)
    luto = oracle.valid_lut(spo, W, H)
    for i in range(B):
        L, R = oracle.synth_pair(W, H, scene, 12345 + i)
        st, D1o, D2o = oracle.process(oracle.params(disp_max=D - 1), L, R)
        assert st == 0
        assert np.array_equal(got["D1"][i].view(np.uint32), D1o.view(np.uint32)) and np.array_equal(got["D2"][i].view(np.uint32), D2o.view(np.uint32)), i
        u8o = oracle.to_u8(D1o)
        assert np.array_equal(got["disparity_u8"][i], u8o.astype(np.float32)), i
        bo, mo, _ = oracle.scan(spo, u8o, luto)
        assert np.allclose(got["scan_bins"][i], bo, rtol=0, atol=1e-4) and np.allclose(got["scan_meta"][i], mo, rtol=0, atol=1e-4), i

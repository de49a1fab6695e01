"""What tests/test_gpu_subpix.py and tests/test_gpu_rigs.py share: the inputs of the sub-pixel tail, one run of its three entry points and the
comparison of their outputs with the definition (tests/subpix_def.py).  TEST INFRASTRUCTURE."""
import numpy as np

import subpix_def as sd
from rigs import tweak_w0                    # (tests/test_gpu_subpix.py takes it from here)

SCAN_TOL = 1e-4                       # device atan2 / sqrt against numpy's: what the existing scan tests allow
MARGIN = 1e-9                         # a bearing this close (in bins) to a bin edge does not decide its bin: that frame's bins are not compared
FORMATS = (sd.F32, sd.I16, sd.I16_SUB)


def random_q(rng, n, H, W):
    """q in 1/16 pixel: fractional noise, faces of constant disparity (the runs the kernel keeps in registers), invalid pixels, pixels at
    q = 112 (w = 0 under tweak_w0), values around the default min_q."""
    q = rng.integers(-40, 2200, (n, H, W))
    for f in range(n):
        for _ in range(12):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            q[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(40, 1900)
    special = rng.random((n, H, W))
    for v, lo in ((-16, 0.00), (31, 0.04), (32, 0.08), (112, 0.12), (33, 0.16)):
        q[(special >= lo) & (special < lo + 0.04)] = v
    return q


def as_format(q, fmt, rng=None):
    """q (1/16 pixel, int) -> an array of the format whose to_q gives q back (I16: q is made a multiple of 16 first)."""
    if fmt == sd.F32:
        a = (q.astype(np.float64) / 16.0).astype(np.float32)
        if rng is not None:                                      # below the rounding step: rint(16 d) must not move
            a = (a.astype(np.float64) + (rng.random(q.shape) - 0.5) * 0.05).astype(np.float32)
        return a
    if fmt == sd.I16:
        return np.floor_divide(q, 16).astype(np.int16)
    return q.astype(np.int16)


def run(sp, cp, fp, maps, want_cloud=True):
    """maps [n][H][W] -> dict of numpy outputs of jn_subpix_costmap, jn_subpix_scan and jn_subpix_point_cloud (first map)."""
    from jackal_navigation_amd import subpix
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = maps.shape
    dD = DeviceArray.from_numpy(maps)
    out = {}
    bins = DeviceArray.from_numpy(np.full((n, sp.bins), 77.0)); meta = DeviceArray.from_numpy(np.full((n, 4), 77.0))
    subpix.subpix_scan(sp, fp, n, dD.ptr, W, H, bins.ptr, meta.ptr)
    out["scan_bins"], out["scan_meta"] = bins.numpy(), meta.numpy()
    if cp is not None:
        bins2 = DeviceArray.from_numpy(np.full((n, sp.bins), 55.0)); meta2 = DeviceArray.from_numpy(np.full((n, 4), 55.0))
        hits = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), 0xABCD, np.uint16))
        grid = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), 77, np.int8))
        subpix.subpix_costmap(sp, cp, fp, n, dD.ptr, W, H, bins2.ptr, meta2.ptr, hits.ptr, grid.ptr)
        out.update(bins=bins2.numpy(), meta=meta2.numpy(), hits=hits.numpy(), grid=grid.numpy())
    if want_cloud:
        out["cloud"] = subpix.subpix_point_cloud(sp, fp, dD.ptr, W, H)
    return out


def check_against_definition(sp, cp, fp, maps, out, what):
    """-> the number of frames whose bins were not compared (a bearing within 1e-9 bins of a bin edge)."""
    n = maps.shape[0]
    left_out = 0
    if "bins" in out:                                             # the costmap call's scan IS the scan call's
        assert np.array_equal(out["bins"], out["scan_bins"]) and np.array_equal(out["meta"], out["scan_meta"]), what
    for f in range(n):
        q, valid = sd.to_q(maps[f], fp.format, fp.min_q)
        bins, meta, edge = sd.scan(sp, q, valid)
        got = out["scan_bins"][f]
        if edge > MARGIN:                                           # no pixel's bin hangs on the last bits of its atan2
            assert np.array_equal(got < sd.EMPTY - 1, bins < sd.EMPTY - 1), (what, f)
            assert np.allclose(got, bins, rtol=0, atol=SCAN_TOL), (what, f)
        else:
            left_out += 1
        assert np.allclose(out["scan_meta"][f], meta, rtol=0, atol=SCAN_TOL), (what, f)
        if cp is not None:
            want = sd.hits(sp, cp, q, valid)
            assert np.array_equal(out["hits"][f], want), (what, f, int((out["hits"][f] != want).sum()))
            g, decided = sd.classify(sp, cp, want, out["bins"][f])
            assert np.array_equal(out["grid"][f] == 100, g == 100), (what, f)
            assert set(np.unique(out["grid"][f])) <= {-1, 0, 100}, (what, f)
            assert np.array_equal(out["grid"][f][decided], g[decided]), (what, f)
    if "cloud" in out:
        q, valid = sd.to_q(maps[0], fp.format, fp.min_q)
        want = sd.cloud(sp, q, valid)
        assert out["cloud"].shape == want.shape and np.array_equal(out["cloud"].view(np.uint32), want.view(np.uint32)), what
    return left_out


def integer_maps(rng, n, H, W):
    m = rng.integers(2, 256, (n, H, W)).astype(np.uint8)
    for f in range(n):
        for _ in range(10):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            m[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(3, 120)
    return m

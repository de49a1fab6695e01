"""What tests/test_gpu_localmap.py and tests/test_gpu_rigs.py share: the inputs of the local map, one update on the handle and on the definition
(tests/localmap_def.py) and the comparison of counts, state, grid and window.  TEST INFRASTRUCTURE."""
import numpy as np

import localmap_def as ld
from rigs import tweak_w0                    # (tests/test_gpu_localmap.py takes it from here)


def random_q(rng, n, H, W):
    """q in 1/16 pixel: noise, faces of constant disparity, bands of slowly varying disparity (what a floor looks like to the run-length
    combine), invalid pixels, pixels at q = 112 (w = 0 under tweak_w0), values around the default min_q."""
    q = rng.integers(-40, 2200 * max(W, 640) // 1280, (n, H, W))
    for f in range(n):
        for _ in range(10):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            q[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(40, 1900)
        y0 = int(rng.integers(0, H))
        q[f, y0:] = (40 + (2100 * W // 1280) * np.arange(H - y0) // (H - y0))[:, None] + rng.integers(0, 2, (H - y0, W))
    special = rng.random((n, H, W))
    for v, lo in ((-16, 0.00), (31, 0.03), (32, 0.06), (112, 0.09), (33, 0.12)):
        q[(special >= lo) & (special < lo + 0.03)] = v
    return q


def as_format(q, fmt):
    """q (1/16 pixel, int) -> an array of the format (I16 drops the fraction)."""
    if fmt == ld.F32:
        return (q.astype(np.float64) / 16.0).astype(np.float32)
    if fmt == ld.I16:
        return np.floor_divide(q, 16).astype(np.int16)
    return q.astype(np.int16)


def gpu_update(m, sp, poses, maps):
    """-> (obst, floor) u16 [n][cy][cx] as the library wrote them (buffers poisoned beforehand)."""
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = maps.shape
    p = m.params
    dD = DeviceArray.from_numpy(maps)
    dO = DeviceArray.from_numpy(np.full((n, p.cells_y, p.cells_x), 0xABCD, np.uint16))
    dF = DeviceArray.from_numpy(np.full((n, p.cells_y, p.cells_x), 0xABCD, np.uint16))
    m.update(sp, poses, dD.ptr, W, H, dO.ptr, dF.ptr)
    out = dO.numpy(), dF.numpy()
    for d in (dD, dO, dF):
        d.free()
    return out


def step(m, ref, sp, poses, maps, what=None):
    """One update on both; counts, state, grid and window compared."""
    o, f = gpu_update(m, sp, poses, maps)
    wo, wf = ref.update(sp, poses, maps)
    assert np.array_equal(o, wo), (what, "obst", int((o != wo).sum()))
    assert np.array_equal(f, wf), (what, "floor", int((f != wf).sum()))
    same_state(m, ref, what)
    return o, f


def same_state(m, ref, what=None):
    L, g = m.read()
    assert L.dtype == np.int16 and g.dtype == np.int8 and L.shape == g.shape == ref.L.shape
    assert np.array_equal(L, ref.L), (what, "L", int((L != ref.L).sum()))
    assert np.array_equal(g, ref.grid()), (what, "grid")
    w = m.window()
    assert w.g0 == ref.g0 and w.origin == (float(ref.g0[0]) * ref.p.resolution, float(ref.g0[1]) * ref.p.resolution), what


def generic_poses(rng, n):
    return [(float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-3.1, 3.1))) for _ in range(n)]

"""What tests/test_gpu_costmap.py and tests/test_gpu_rigs.py share: the inputs of the obstacle costmap, one run of it behind the scan of the same
maps and the comparison with the definition (tests/costmap_def.py).  TEST INFRASTRUCTURE."""
import numpy as np

import costmap_def as cd
from rigs import tweak_w0                    # (tests/test_gpu_costmap.py takes it from here)


def run_costmap(sp, cp, maps, lut, with_bins=True):
    """maps [n][H][W] u8 (numpy) -> (hits, grid, bins) from jn_obstacle_costmap, the bins from the scan of the same maps with the same rule."""
    from jackal_navigation_amd import costmap, node
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = maps.shape
    dD = DeviceArray.from_numpy(maps)
    bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    if cp.from_cloud:
        node.obstacle_scan_cloud(sp, n, dD.ptr, W, H, bins.ptr, meta.ptr)
    else:
        node.obstacle_scan(sp, n, dD.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
    hits = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), 0xABCD, np.uint16))
    grid = DeviceArray.from_numpy(np.full((n, cp.cells_y, cp.cells_x), 77, np.int8))
    costmap.obstacle_costmap(sp, cp, n, dD.ptr, None if cp.from_cloud else lut.ptr, W, H, bins.ptr if with_bins else None, hits.ptr, grid.ptr)
    return hits.numpy(), grid.numpy(), bins.numpy()


def check_against_definition(sp, cp, maps, lut_np, hits, grid, bins, what):
    for f in range(maps.shape[0]):
        want = cd.hits(sp, cp, maps[f], lut_np)
        assert np.array_equal(hits[f], want), (what, f, int((hits[f] != want).sum()))
        g, decided = cd.classify(sp, cp, want, None if bins is None else bins[f])
        assert np.array_equal(grid[f] == 100, g == 100), (what, f)
        assert set(np.unique(grid[f])) <= {-1, 0, 100}, (what, f)
        assert np.array_equal(grid[f][decided], g[decided]), (what, f, int((grid[f][decided] != g[decided]).sum()))
        if bins is None:
            assert not (grid[f] == 0).any(), (what, f)


def random_maps(rng, n, H, W):
    """Every disparity value occurs, 0 / 1 / 2 / 255 and 7 (w = 0 under tweak_w0) often; columns of constant disparity (the runs the
    kernel keeps in registers) next to pixel noise (a run of one)."""
    m = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    special = rng.random((n, H, W))
    for v, lo in ((0, 0.00), (1, 0.05), (2, 0.10), (255, 0.15), (7, 0.20)):
        m[(special >= lo) & (special < lo + 0.05)] = v
    for f in range(n):
        for _ in range(12):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            m[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(3, 120)
    return m

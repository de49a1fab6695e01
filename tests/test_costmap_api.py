"""The obstacle costmap's C ABI (include/jn_costmap.h) and its Python mirror: exports, struct layout, defaults, argument checking,
the OccupancyGrid message.  No GPU needed; the compute lives in tests/test_gpu_costmap.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "jn_costmap.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(jn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_by_both_libraries(jn):
    from jackal_navigation_amd import costmap
    declared = _declared_functions()
    assert declared == sorted(costmap.COSTMAP_EXPORTS) == sorted(jn.COSTMAP_EXPORTS)
    assert len(declared) == 5
    lib = jn.load()
    assert not [n for n in declared if not hasattr(lib, n)]
    with jn.hooks_library() as hooks:
        assert hooks is not lib
        assert not [n for n in declared if not hasattr(hooks, n)]


def test_version_says_0_4(jn):
    assert jn.load().jn_version() == b"jn_stereo 0.4 (gfx950)"


def test_struct_layout_and_defaults(jn):
    from jackal_navigation_amd import costmap
    assert C.sizeof(costmap.CostmapParams) == 3 * 8 + 4 * 4 == 40
    assert costmap.CostmapParams.resolution.offset == 16 and costmap.CostmapParams.cells_x.offset == 24 and costmap.CostmapParams.from_cloud.offset == 36
    cp = costmap.costmap_params()
    assert (cp.origin_x, cp.origin_y, cp.resolution, cp.cells_x, cp.cells_y, cp.min_hits, cp.from_cloud) == (0.0, -3.2, 0.05, 128, 128, 3, 0)
    assert costmap.costmap_params(cells_x=7, from_cloud=1).cells_x == 7
    with pytest.raises(AttributeError):
        costmap.costmap_params(cellsx=7)
    # the header's constants and the module's agree
    text = open(os.path.join(ROOT, "include", "jn_costmap.h")).read()
    assert int(re.search(r"#define JN_COSTMAP_MAX_CELLS (\d+)", text).group(1)) == costmap.MAX_CELLS == 512
    assert (costmap.OCCUPIED, costmap.FREE, costmap.UNKNOWN) == (100, 0, -1)


BAD = [dict(resolution=0.0), dict(resolution=-0.05), dict(resolution=float("nan")), dict(resolution=float("inf")), dict(origin_x=float("nan")),
       dict(cells_x=0), dict(cells_x=513), dict(cells_y=0), dict(cells_y=513), dict(cells_x=-4), dict(min_hits=0), dict(min_hits=-1),
       dict(from_cloud=2), dict(from_cloud=-1)]


def test_invalid_arguments_are_refused_before_the_device_is_touched(jn):
    """Every check comes ahead of hipSetDevice: on a machine without a GPU these calls still say JN_ERR_INVALID, not JN_ERR_NO_DEVICE."""
    from jackal_navigation_amd import costmap, node, _lib
    L = costmap._bind()
    sp = node.scan_params(320, 180)
    p = 4096                                                # never dereferenced: the calls are refused first
    for kw in BAD:
        cp = costmap.costmap_params(**kw)
        assert L.jn_obstacle_costmap(0, C.byref(sp), C.byref(cp), 1, p, p, 320, 180, None, p, p) == _lib.JN_ERR_INVALID, kw
    cp = costmap.costmap_params()
    for args in ((None, C.byref(cp), 1, p, p, 320, 180, None, p, p), (C.byref(sp), None, 1, p, p, 320, 180, None, p, p),
                 (C.byref(sp), C.byref(cp), 0, p, p, 320, 180, None, p, p), (C.byref(sp), C.byref(cp), 1, None, p, 320, 180, None, p, p),
                 (C.byref(sp), C.byref(cp), 1, p, None, 320, 180, None, p, p),          # the LUT rule without a LUT
                 (C.byref(sp), C.byref(cp), 1, p, p, 0, 180, None, p, p), (C.byref(sp), C.byref(cp), 1, p, p, 320, 0, None, p, p),
                 (C.byref(sp), C.byref(cp), 1, p, p, 320, 180, None, None, p), (C.byref(sp), C.byref(cp), 1, p, p, 320, 180, None, p, None)):
        assert L.jn_obstacle_costmap(0, *args) == _lib.JN_ERR_INVALID, args
    sp_bad = node.scan_params(320, 180)
    sp_bad.bins = 0
    assert L.jn_obstacle_costmap(0, C.byref(sp_bad), C.byref(cp), 1, p, p, 320, 180, None, p, p) == _lib.JN_ERR_INVALID
    sp_bad.bins = 1025
    assert L.jn_obstacle_costmap(0, C.byref(sp_bad), C.byref(cp), 1, p, p, 320, 180, None, p, p) == _lib.JN_ERR_INVALID
    # handle-bound calls: no handle, no communicator
    assert L.jn_elas_attach_costmap(None, 0, C.byref(cp), p, p) == _lib.JN_ERR_INVALID
    assert L.jn_sgm_attach_costmap(None, 0, C.byref(cp), p, p) == _lib.JN_ERR_INVALID
    assert L.jn_costmap_allreduce(None, C.byref(sp), C.byref(cp), 1, None, p, p) == _lib.JN_ERR_INVALID
    with pytest.raises(TypeError):
        costmap.attach(object(), 0, cp, p, p)


def test_compute_without_a_device_fails_loudly(jn):
    from jackal_navigation_amd import costmap, node, _lib
    from jackal_navigation_amd.device import device_count
    if device_count() > 0:
        pytest.skip("a GPU is present")
    sp = node.scan_params(320, 180)
    for fc in (0, 1):
        with pytest.raises(_lib.JnError) as e:
            costmap.obstacle_costmap(sp, costmap.costmap_params(from_cloud=fc), 1, 4096, 4096, 320, 180, None, 4096, 4096)
        assert e.value.status == _lib.JN_ERR_NO_DEVICE


def test_occupancy_grid_message_fields(jn):
    from jackal_navigation_amd import costmap
    cp = costmap.costmap_params(cells_x=4, cells_y=3, resolution=0.25, origin_x=1.0, origin_y=-0.5)
    grid = np.array([[-1, 0, 0, 100], [0, 100, -1, -1], [-1, -1, -1, 0]], np.int8)
    m = costmap.occupancy_grid_message(grid, cp, seq=7)
    assert m["header"] == {"seq": 7, "frame_id": "jackal"}
    info = m["info"]
    assert info["resolution"] == np.float32(0.25) and info["resolution"].dtype == np.float32          # float32 in nav_msgs/MapMetaData
    assert (info["width"], info["height"]) == (4, 3)                                                    # width = cells along x = a row of data
    assert info["origin"]["position"] == {"x": 1.0, "y": -0.5, "z": 0.0} and info["origin"]["orientation"]["w"] == 1.0
    assert m["data"].dtype == np.int8 and m["data"].tolist() == [-1, 0, 0, 100, 0, 100, -1, -1, -1, -1, -1, 0]    # row-major, x along the row
    with pytest.raises(ValueError):
        costmap.occupancy_grid_message(grid.T, cp)


def test_the_numpy_definition_on_a_hand_made_case(jn):
    """The checker itself: three pixels at the same disparity land where hand arithmetic puts them, and the free / unknown split
    follows the bins."""
    from jackal_navigation_amd import costmap, node
    import costmap_def as cd
    W, H = 64, 48
    sp = node.scan_params(W, H)
    cp = costmap.costmap_params(resolution=0.5, cells_x=8, cells_y=8, origin_x=0.0, origin_y=-2.0, min_hits=2, from_cloud=1)
    sp.gp_height_thresh = -1e9                               # nothing is ground
    disp = np.zeros((H, W), np.uint8)
    disp[20:23, 30] = 9
    X, Y, Z, ok = cd.reproject(sp, disp)
    assert ok[20, 30] and np.isfinite(X[20, 30])
    ix, iy = int(np.floor((X[20, 30] - 0.0) / 0.5)), int(np.floor((Y[20, 30] + 2.0) / 0.5))
    assert 0 <= ix < 8 and 0 <= iy < 8
    h = cd.hits(sp, cp, disp, None)
    assert h.sum() == 3 and h[iy, ix] == 3
    bins = np.full(sp.bins, cd.EMPTY)
    grid, decided = cd.classify(sp, cp, h, bins)
    assert grid[iy, ix] == 100 and (grid == 0).sum() == 0 and (grid == -1).sum() == 63
    bins[:] = 100.0                                          # a return far away in every direction: every cell inside the fan is free
    grid, decided = cd.classify(sp, cp, h, bins)
    assert grid[iy, ix] == 100 and (grid == 0).sum() > 20 and decided[iy, ix]
    grid, _ = cd.classify(sp, cp, h, None)
    assert (grid == 0).sum() == 0

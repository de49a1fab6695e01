"""The sub-pixel navigation tail's C ABI (include/jn_subpix.h), its Python mirror and its numpy definition (tests/subpix_def.py): exports,
struct layout, defaults, argument checking; the definition on its edge values, its anchor in tests/costmap_def.py, and the accuracy
claim the mode exists for.  No GPU needed; the compute lives in tests/test_gpu_subpix.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import costmap_def as cd
import subpix_def as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "jn_subpix.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(jn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_by_both_libraries(jn):
    from jackal_navigation_amd import subpix
    declared = _declared_functions()
    assert declared == sorted(subpix.SUBPIX_EXPORTS) == sorted(jn.SUBPIX_EXPORTS)
    assert len(declared) == 6
    lib = jn.load()
    assert not [n for n in declared if not hasattr(lib, n)]
    with jn.hooks_library() as hooks:
        assert hooks is not lib
        assert not [n for n in declared if not hasattr(hooks, n)]
    for name in ("SubpixParams", "subpix_scan", "subpix_costmap", "subpix_point_cloud"):
        assert hasattr(jn, name), name
    assert hasattr(jn.Elas, "attach_subpix") and hasattr(jn.Sgm, "attach_subpix")


def test_version_is_unchanged(jn):
    assert jn.load().jn_version() == b"jn_stereo 0.4 (gfx950)"


def test_struct_layout_defaults_and_constants(jn):
    from jackal_navigation_amd import subpix, ground, costmap
    assert C.sizeof(subpix.SubpixParams) == 8 and subpix.SubpixParams.min_q.offset == 4
    assert C.sizeof(costmap.CostmapParams) == 40                       # no existing struct changed size
    for fmt in (subpix.F32, subpix.I16, subpix.I16_SUB):
        fp = subpix.subpix_params(fmt)
        assert (fp.format, fp.min_q) == (fmt, 32)
    assert subpix.subpix_params(subpix.I16, min_q=48).min_q == 48
    with pytest.raises(AttributeError):
        subpix.subpix_params(subpix.I16, minq=48)
    assert (subpix.F32, subpix.I16, subpix.I16_SUB) == (ground.F32, ground.I16, ground.I16_SUB) == (sd.F32, sd.I16, sd.I16_SUB)
    text = open(os.path.join(ROOT, "include", "jn_subpix.h")).read()
    m = re.search(r"JN_DISP_F32 = (\d+), JN_DISP_I16 = (\d+), JN_DISP_I16_SUB = (\d+)", text)
    assert tuple(int(x) for x in m.groups()) == (0, 1, 2)
    gtext = open(os.path.join(ROOT, "include", "jn_ground.h")).read()
    assert 16 * int(re.search(r"#define JN_GROUND_MAX_SIDE (\d+)", gtext).group(1)) == subpix.MAX_Q == sd.MAX_Q


BAD_CP = [dict(resolution=0.0), dict(resolution=float("nan")), dict(origin_y=float("inf")), dict(cells_x=0), dict(cells_x=513), dict(cells_y=0),
          dict(cells_y=513), dict(min_hits=0)]
BAD_FP = [dict(format=-1), dict(format=3), dict(min_q=-1), dict(min_q=16 * 4096 + 1)]


def test_invalid_arguments_are_refused_before_the_device_is_touched(jn):
    """Every check comes ahead of hipSetDevice: on a machine without a GPU these calls still say JN_ERR_INVALID, not JN_ERR_NO_DEVICE."""
    from jackal_navigation_amd import costmap, node, subpix, _lib
    L = subpix._bind()
    INV = _lib.JN_ERR_INVALID
    sp, cp, fp = node.scan_params(320, 180), costmap.costmap_params(), subpix.subpix_params(subpix.F32)
    S, Cp, F = C.byref(sp), C.byref(cp), C.byref(fp)
    p = 4096                                                # never dereferenced: the calls are refused first
    cnt = C.c_int64(0)
    for kw in BAD_FP:
        bad = subpix.subpix_params(subpix.I16)
        for k, v in kw.items():
            setattr(bad, k, v)
        assert L.jn_subpix_scan(0, S, C.byref(bad), 1, p, 320, 180, p, p) == INV, kw
        assert L.jn_subpix_costmap(0, S, Cp, C.byref(bad), 1, p, 320, 180, p, p, p, p) == INV, kw
        assert L.jn_subpix_point_cloud(0, S, C.byref(bad), p, 320, 180, p, C.byref(cnt)) == INV, kw
    for kw in BAD_CP:
        assert L.jn_subpix_costmap(0, S, C.byref(costmap.costmap_params(**kw)), F, 1, p, 320, 180, p, p, p, p) == INV, kw
    for args in ((None, F, 1, p, 320, 180, p, p), (S, None, 1, p, 320, 180, p, p), (S, F, 0, p, 320, 180, p, p), (S, F, -3, p, 320, 180, p, p),
                 (S, F, 1, None, 320, 180, p, p), (S, F, 1, p, 0, 180, p, p), (S, F, 1, p, 320, 0, p, p), (S, F, 1, p, 320, 180, None, p),
                 (S, F, 1, p, 320, 180, p, None)):
        assert L.jn_subpix_scan(0, *args) == INV, args
    for args in ((None, Cp, F, 1, p, 320, 180, p, p, p, p), (S, None, F, 1, p, 320, 180, p, p, p, p), (S, Cp, None, 1, p, 320, 180, p, p, p, p),
                 (S, Cp, F, 0, p, 320, 180, p, p, p, p), (S, Cp, F, 1, None, 320, 180, p, p, p, p), (S, Cp, F, 1, p, 0, 180, p, p, p, p),
                 (S, Cp, F, 1, p, 320, -1, p, p, p, p), (S, Cp, F, 1, p, 320, 180, None, p, p, p), (S, Cp, F, 1, p, 320, 180, p, None, p, p),
                 (S, Cp, F, 1, p, 320, 180, p, p, None, p), (S, Cp, F, 1, p, 320, 180, p, p, p, None)):
        assert L.jn_subpix_costmap(0, *args) == INV, args
    for args in ((None, F, p, 320, 180, p, C.byref(cnt)), (S, None, p, 320, 180, p, C.byref(cnt)), (S, F, None, 320, 180, p, C.byref(cnt)),
                 (S, F, p, 0, 180, p, C.byref(cnt)), (S, F, p, 320, 0, p, C.byref(cnt)), (S, F, p, 320, 180, None, C.byref(cnt)),
                 (S, F, p, 320, 180, p, None)):
        assert L.jn_subpix_point_cloud(0, *args) == INV, args
    for b in (0, 1025, -1):
        sp_bad = node.scan_params(320, 180)
        sp_bad.bins = b
        assert L.jn_subpix_scan(0, C.byref(sp_bad), F, 1, p, 320, 180, p, p) == INV
        assert L.jn_subpix_costmap(0, C.byref(sp_bad), Cp, F, 1, p, 320, 180, p, p, p, p) == INV
    # handle-bound calls: no handle (the slot checks need one and live in the GPU tests)
    assert L.jn_elas_attach_subpix(None, 0, Cp, p, p, p, p) == INV
    assert L.jn_sgm_attach_subpix(None, 0, Cp, p, p, p, p) == INV
    assert L.jn_elas_attach_subpix(None, 0, None, None, None, None, None) == INV
    with pytest.raises(TypeError):
        subpix.attach(object(), 0, cp, p, p, p, p)


def test_compute_without_a_device_fails_loudly(jn):
    from jackal_navigation_amd import costmap, node, subpix, _lib
    from jackal_navigation_amd.device import device_count
    if device_count() > 0:
        pytest.skip("a GPU is present")
    sp = node.scan_params(320, 180)
    for fmt in (subpix.F32, subpix.I16, subpix.I16_SUB):
        with pytest.raises(_lib.JnError) as e:
            subpix.subpix_costmap(sp, costmap.costmap_params(), subpix.subpix_params(fmt), 1, 4096, 320, 180, 4096, 4096, 4096, 4096)
        assert e.value.status == _lib.JN_ERR_NO_DEVICE
        with pytest.raises(_lib.JnError) as e:
            subpix.subpix_scan(sp, subpix.subpix_params(fmt), 1, 4096, 320, 180, 4096, 4096)
        assert e.value.status == _lib.JN_ERR_NO_DEVICE


def test_to_q_on_the_edge_values():
    import ground_def as gd
    f = np.array([2.0, 2.03125, 2.09375, 2.15625, 1.96875, 1.96874, np.nan, np.inf, -np.inf, -10.0, -1.0, 0.0, 4096.0, 4096.03125, 4096.04, 1e30],
                 np.float32)
    q, v = sd.to_q(f, sd.F32)
    # 16 d = 32, 32.5 -> 32, 33.5 -> 34, 34.5 -> 34 (ties to even); 31.5 -> 32 is valid, 31.4998 -> 31 is not
    assert q[:5].tolist() == [32, 32, 34, 34, 32] and v[:5].all()
    assert not v[5:12].any() and (q[5:12] == 0).all()
    # 16 * 4096 is the last valid value; 65536.5 ties to it; 65536.64 -> 65537 is out
    assert v[12] and q[12] == 65536 and v[13] and q[13] == 65536 and not v[14] and not v[15]
    q, v = sd.to_q(f, sd.F32, min_q=0)
    assert v[11] and q[11] == 0 and not v[9] and not v[10]
    i = np.array([-16, -1, 0, 1, 2, 31, 32, 33, 255, 4096, 4097, 32767, -32768], np.int16)
    q, v = sd.to_q(i, sd.I16)
    assert q.tolist() == [16 * int(x) for x in i] and v.tolist() == [False] * 4 + [True] * 6 + [False] * 3
    q, v = sd.to_q(i, sd.I16_SUB)
    assert q.tolist() == [int(x) for x in i] and v.tolist() == [False] * 6 + [True] * 6 + [False]
    assert sd.to_q(np.array([32767], np.int16), sd.I16_SUB)[1][0]                 # int16 cannot exceed 16 * 4096 in 1/16 pixel
    # the rule is jn_ground.h's
    for fmt, a in ((sd.F32, f), (sd.I16, i), (sd.I16_SUB, i)):
        for md in (0, 2, 5):
            qa, va = sd.to_q(a, fmt, 16 * md)
            qb, vb = gd.to_q(a, fmt, md)
            assert np.array_equal(va, vb) and np.array_equal(qa[va], qb[vb])


def _integer_maps(rng, n, H, W):
    m = rng.integers(2, 256, (n, H, W)).astype(np.uint8)
    for f in range(n):
        for _ in range(8):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            m[f, y0:y1 + 1, x0:x1 + 1] = rng.integers(3, 120)
    return m


def test_the_anchor_property_of_the_definition(jn):
    """On integer maps with 2 <= d <= 255 the definition IS the existing one: hits and grid equal costmap_def's (from_cloud = 1) bit for bit
    in all three formats, the bins classify the same cells, and the cloud holds the float32 of costmap_def's points in i-outer order."""
    from jackal_navigation_amd import costmap, node
    W, H, n = 120, 67, 2
    rng = np.random.default_rng(21)
    sp = node.scan_params(W, H)
    sp.crop_offset_x, sp.crop_offset_y = 3, 5
    sp.Q[15] = -(sp.Q[14] * 7.0)                               # d = 7 has w = 0
    cp = costmap.costmap_params(from_cloud=1, min_hits=2)
    maps = _integer_maps(rng, n, H, W)
    assert (maps == 7).any()
    for f in range(n):
        want = cd.hits(sp, cp, maps[f], None)
        outs = []
        for fmt, arr in ((sd.F32, maps[f].astype(np.float32)), (sd.I16, maps[f].astype(np.int16)), (sd.I16_SUB, maps[f].astype(np.int16) * 16)):
            q, v = sd.to_q(arr, fmt)
            assert v.all() and np.array_equal(q, maps[f].astype(np.int64) * 16)
            h = sd.hits(sp, cp, q, v)
            assert np.array_equal(h, want), fmt
            bins, meta, _ = sd.scan(sp, q, v)
            outs.append((bins, meta))
            X, Y, Z, ok = cd.reproject(sp, maps[f])
            pts = sd.cloud(sp, q, v)
            assert pts.shape == (W * H, 3) and pts.dtype == np.float32
            ref = np.stack([np.where(ok, X, 0), np.where(ok, Y, 0), np.where(ok, Z, 0)], -1).transpose(1, 0, 2).reshape(-1, 3).astype(np.float32)
            assert np.array_equal(pts.view(np.uint32), ref.view(np.uint32))
            assert (pts[~ok.T.reshape(-1)] == 0).all()
        assert want.sum() > 0
        for b, m in outs[1:]:
            assert np.array_equal(b, outs[0][0]) and np.array_equal(m, outs[0][1])
        assert (outs[0][0] < sd.EMPTY - 1).sum() > 10 and outs[0][1][0] < outs[0][1][1] and outs[0][1][2] < outs[0][1][3]


def test_an_all_invalid_map_leaves_the_initial_values(jn):
    from jackal_navigation_amd import costmap, node
    sp, cp = node.scan_params(64, 48), costmap.costmap_params()
    q, v = sd.to_q(np.full((48, 64), -10.0, np.float32), sd.F32)
    assert not v.any()
    bins, meta, _ = sd.scan(sp, q, v)
    assert (bins == sd.EMPTY).all() and meta.tolist() == [400.0, -400.0, 1e9, -500.0]
    h = sd.hits(sp, cp, q, v)
    g, _ = sd.classify(sp, cp, h, bins)
    assert h.sum() == 0 and (g == -1).all() and sd.cloud(sp, q, v).shape == (0, 3)


def wall_errors(sp, W, H, distance):
    """Median over the bins of |range - true range| for a fronto-parallel wall `distance` metres ahead, through the definition, with the
    true fractional disparity (a) rounded to the mono8 map's integer, (b) rounded to 1/16 pixel."""
    qw, d = sd.wall_q(sp, W, H, distance)
    valid = np.ones((H, W), bool)
    truth, _, _ = sd.scan(sp, np.full((H, W), 16.0 * d), valid)
    u8 = np.rint(np.full((H, W), d))                               # jn_disparity_to_u8 / jn_sgm_disparity_to_u8: round half to even
    coarse, _, _ = sd.scan(sp, 16.0 * u8, valid)
    fine, _, _ = sd.scan(sp, qw, valid)
    hit = truth < sd.EMPTY - 1
    assert hit.sum() > 50 and np.array_equal(hit, coarse < sd.EMPTY - 1) and np.array_equal(hit, fine < sd.EMPTY - 1)
    return float(np.median(np.abs(coarse[hit] - truth[hit]))), float(np.median(np.abs(fine[hit] - truth[hit]))), d


def test_fractional_disparities_put_a_wall_where_it_is(jn):
    """The reason the mode exists: the shipped rig at the node's 320x180, walls at 1.0 / 1.6 / 3.0 / 5.0 m.  The range the scan reports
    from the 1/16-pixel disparity is at least 4x nearer the truth than from the rounded mono8 value at 3 m, and better at every distance."""
    from jackal_navigation_amd import node
    W, H = 320, 180
    sp = node.scan_params(W, H)
    err = {dist: wall_errors(sp, W, H, dist) for dist in (1.0, 1.6, 3.0, 5.0)}
    assert abs(err[3.0][2] - 7.276) < 0.01                        # the issue's 7.3 px at 3 m
    for dist, (coarse, fine, d) in err.items():
        assert fine < coarse, (dist, coarse, fine)
    coarse, fine, _ = err[3.0]
    assert coarse > 0.08 and fine * 4 <= coarse, (coarse, fine)
    assert err[5.0][0] > 0.3 and err[5.0][1] < 0.05

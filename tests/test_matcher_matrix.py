"""The matcher matrix without a GPU: tests/matcher_cases.py launches every instantiation of the matchers' kernels that the library holds, every
saturation / 16-bit case really reaches its edge (by the oracle), and the ABI refuses what lies just outside the parameter ranges."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import matcher_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def binary_instantiations(lib_path, families=None):
    """{family: set of 'k_name<args>'} of the kernels in a build of the library, from the host-side launch stubs"""
    out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    found = {}
    for name in re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", out):
        family = name.split("<")[0]
        if families is None or family in families:
            found.setdefault(family, set()).add(name)
    return found


def test_the_table_launches_every_matcher_kernel_in_the_library(jn):
    from jackal_navigation_amd import _lib
    in_binary = binary_instantiations(_lib.LIB_PATH, mc.MATCHER_FAMILIES)
    assert sorted(in_binary) == sorted(mc.MATCHER_FAMILIES), "a kernel family is gone from the library (or nm's output changed): %s" % sorted(in_binary)
    binary = set().union(*in_binary.values())
    table = mc.table_instantiations()
    assert not binary - table, "in the library, launched by no case of tests/matcher_cases.py: %s" % sorted(binary - table)
    assert not table - binary, "the dispatch restated in tests/matcher_cases.py names kernels the library does not hold: %s" % sorted(table - binary)
    # k_sw_w: 12 image forms are what the release library's cases reach (it ignores JN_SGM_NS / JN_SGM_LQ): D = 64, 128, 256 x downward / final x
    # byte / 16-bit; 12 volume forms, the same product (the volume path has no JN_SGM_NS / JN_SGM_LQ forms); 44 in the binary: the image path's 8
    # layouts (D = 64 and 128 with 2, 4, 8 strips, D = 256 with 8 and with 4 lanes per pixel) x 4 = 32, and the 12 volume forms
    sw_w = lambda names, vol: [k for k in names if k.startswith("k_sw_w<") and k.endswith(", %s>" % vol)]
    release = set().union(*(mc.sgm_instantiations(c) for c in mc.SGM_CASES))
    volume = set().union(*(mc.sgm_instantiations(c, volume=True) for c in mc.SGM_VOLUME_CASES))
    assert len(sw_w(release, "false")) == 12 and len(sw_w(volume, "true")) == 12 and not sw_w(release, "true") and not sw_w(volume, "false")
    assert len(sw_w(binary, "false")) == 32 and len(sw_w(binary, "true")) == 12 and len([k for k in binary if k.startswith("k_sw_w")]) == 44


def test_the_hooks_build_holds_the_same_kernels(jn):
    from jackal_navigation_amd import _lib
    assert binary_instantiations(_lib.HOOKS_LIB_PATH, mc.MATCHER_FAMILIES) == binary_instantiations(_lib.LIB_PATH, mc.MATCHER_FAMILIES)


def test_case_ids_are_unique():
    for cases in (mc.SGM_CASES, mc.BM_CASES):
        assert len({mc.case_id(c) for c in cases}) == len(cases)


@pytest.fixture(scope="module")
def sgm():
    from oracle.binding import SgmOracle
    return SgmOracle()


EDGE_CASES = [c for c in mc.SGM_CASES if c.edge] + [c for _, c in mc.SGM_HOOKS_CASES]


@pytest.mark.parametrize("c", EDGE_CASES, ids=[mc.case_id(c) + "-" + "+".join(c.edge) for c in EDGE_CASES])
def test_sgm_edge_cases_reach_their_edge(sgm, oracle, c):
    """A saturation case whose images never drive a path value to 6 cap + P2, or a 16-bit case whose sums stay below 256, tests nothing"""
    Ls, Rs = mc.images(c, oracle)
    m, _, top = mc.path_excess(sgm, Ls[0], Rs[0], c.D, c.kw)
    assert not mc.sgm_edges(c, m, top), (c.why, "not reached: %s" % mc.sgm_edges(c, m, top), "largest L_r %d" % top)
    assert top <= 255
    wide_forms = {k.split(", ")[4] for k in mc.sgm_instantiations(c) if k.startswith("k_sw_w")}
    assert wide_forms == ({"true"} if "wide" in c.edge else {"false"})


def test_worst_case_block_pairs_are_what_they_claim(sgm):
    from oracle.binding import BmOracle
    bm = BmOracle()
    L, R = mc.PAIRS["saw"](32, 20, 0)
    gL, gR = sgm.prefilter(L, 31), sgm.prefilter(R, 31)
    assert (gL == 62).all() and (gR == 0).all()
    for x, y, d in ((0, 0, 0), (31, 19, 255), (16, 10, 7), (5, 3, 31)):
        for side in (0, 1):
            assert bm.cost(gL, gR, 4, side, x, y, d) == 81 * 62 and bm.cost(gL, gR, 4, side, x, y, d, squared=True) == 81 * 62 * 62
    L, R = mc.PAIRS["peak"](32, 20, 0)
    gL, gR = sgm.prefilter(L, 31), sgm.prefilter(R, 31)
    assert (gL == 62).all() and (gR[:, 13:22] == 62).all() and (gR[:, :13] == 0).all() and (gR[:, 22:] == 0).all()
    for x in range(17, 32):
        costs = [bm.cost(gL, gR, 4, 0, x, 10, d, squared=True) for d in range(32)]
        assert costs[x - 17] == 0 and sorted(costs)[1] == 9 * 62 * 62 and max(costs) == 81 * 62 * 62
    for sq in (0, 1):
        disp = bm.process(bm.params(256, 4, 31, 1, 0, sq), *mc.PAIRS["saw"](32, 20, 0))
        assert (disp == 0).all()                                   # every candidate ties on both sides: d = 0 wins and passes the L/R check


# ---- the ABI's parameter ranges: checked before the device is looked for, so the refusals need no GPU ----
def _sgm_create(jn, **kw):
    h = C.c_void_p()
    return jn.load().jn_sgm_create(C.byref(jn.Sgm.parameters(**kw)), 64, 48, 1, 0, C.byref(h))


def _bm_create(jn, **kw):
    h = C.c_void_p()
    return jn.load().jn_bm_create(C.byref(jn.Bm.parameters(**kw)), 64, 48, 1, 0, C.byref(h))


def test_sgm_create_refuses_what_lies_outside_the_ranges(jn):
    from jackal_navigation_amd import _lib
    for kw in ({"num_disparities": 64, "P2": 70, "prefilter_cap": 31},           # 6 cap + P2 = 256
               {"num_disparities": 64, "P2": 250, "prefilter_cap": 1},
               {"num_disparities": 64, "P1": 61, "P2": 60},                       # P2 < P1
               {"num_disparities": 64, "P1": -1},
               {"num_disparities": 64, "prefilter_cap": 0}, {"num_disparities": 64, "prefilter_cap": 32, "P2": 10},
               {"num_disparities": 32}, {"num_disparities": 96}, {"num_disparities": 192}, {"num_disparities": 512}, {"num_disparities": 0}):
        assert _sgm_create(jn, **kw) == _lib.JN_ERR_UNSUPPORTED, kw
    h = C.c_void_p()
    p = jn.Sgm.parameters(num_disparities=64)
    for W, H, mb in ((7, 8, 1), (8, 7, 1), (8193, 8, 1), (8, 8, 0)):
        assert jn.load().jn_sgm_create(C.byref(p), W, H, mb, 0, C.byref(h)) == _lib.JN_ERR_INVALID, (W, H, mb)


def test_bm_create_refuses_what_lies_outside_the_ranges(jn):
    from jackal_navigation_amd import _lib
    for kw in ({"num_disparities": 264}, {"num_disparities": 36}, {"num_disparities": 0}, {"block_radius": 1}, {"block_radius": 5},
               {"prefilter_cap": 0}, {"prefilter_cap": 32}, {"cost_function": 2},
               {"num_disparities": 40, "cost_function": 1}, {"num_disparities": 8, "cost_function": 1}):       # the matrix-core path tiles by 32
        assert _bm_create(jn, **kw) == _lib.JN_ERR_UNSUPPORTED, kw
    h = C.c_void_p()
    p = jn.Bm.parameters()
    for W, H, mb in ((7, 8, 1), (8, 7, 1), (8, 8193, 1), (8, 8, 0)):
        assert jn.load().jn_bm_create(C.byref(p), W, H, mb, 0, C.byref(h)) == _lib.JN_ERR_INVALID, (W, H, mb)


def test_the_tables_parameters_are_inside_the_ranges():
    """every case is a valid call of the ABI (the GPU file shows they are ACCEPTED: P2 = 249, 6 cap + P2 = 255, D = 8)"""
    for c in mc.SGM_CASES + [c for _, c in mc.SGM_HOOKS_CASES] + mc.SGM_VOLUME_CASES:       # (a volume case: 6 cap <= 255 - P2 bounds its bytes too)
        P1, P2, cap = c.kw.get("P1", 10), c.kw.get("P2", 60), c.kw.get("prefilter_cap", 31)
        assert c.D in (64, 128, 256) and 0 <= P1 <= P2 and 1 <= cap <= 31 and 6 * cap + P2 <= 255 and c.W >= 8 and c.H >= 8, c
    for c in mc.BM_CASES:
        assert 8 <= c.D <= 256 and c.D % (32 if c.kw.get("cost_function") else 8) == 0 and 2 <= c.kw.get("block_radius", 4) <= 4 and c.W >= 8 and c.H >= 8, c
    assert {(c.D, c.kw["block_radius"]) for c in mc.BM_SSD_CASES} >= {(D, r) for D in range(32, 257, 32) for r in (2, 3, 4)}
    assert {(c.D, c.kw["block_radius"]) for c in mc.BM_SAD_CASES} >= {(D, r) for D in mc.BM_SAD_DS for r in (2, 3, 4)}

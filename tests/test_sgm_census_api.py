"""The census / Hamming cost of the SGM mode (include/jn_sgm_cost.h, JN_SGM_COST_CENSUS) without a GPU: the anchor of its scalar definition
(tests/sgm_census_def.py), its invariance under a strictly increasing grey-scale change, the constant, argument checking and the kernels
the two builds of the library hold.  The compute lives in tests/test_gpu_sgm_census.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import matcher_cases as mc
import sgm_census_def as cs
import sgm_cost_def as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition's anchors ----
@pytest.mark.parametrize("r", [2, 3, 4])
def test_census_volume_equals_the_literal_loop(r):
    rng = np.random.default_rng(10 + r)
    W, H, D = 11, 9, 16                                        # narrower than D: the clamped centre column and every window clamp
    L, R = rng.integers(0, 6, (H, W)).astype(np.uint8), rng.integers(0, 6, (H, W)).astype(np.uint8)      # few grey levels: many ties
    for cost_max in (7, 127):
        got = cs.census_volume(L, R, D, r, cost_max)
        assert got.dtype == np.uint8 and np.array_equal(got, cs.census_volume_literal(L, R, D, r, cost_max))
    assert cs.census_volume(L, R, D, r, 127).max() > 7         # ... so the clamp at 7 did bite
    assert cs.census_volume(L, R, D, r, 127).max() <= cs.bits(r)


def test_windows_and_bits():
    assert [cs.window(r) for r in (2, 3, 4)] == [(2, 2), (3, 3), (4, 3)]
    assert [cs.bits(r) for r in (2, 3, 4)] == [24, 48, 62]
    I = np.arange(35, dtype=np.uint8).reshape(5, 7)
    for r in (2, 3, 4):
        assert cs.census(I, *cs.window(r)).shape == (5, 7, cs.bits(r))
    assert not cs.census(np.full((6, 9), 200, np.uint8), 4, 3).any()          # strictly less: a constant image has empty signatures
    assert not cs.census_volume(np.full((6, 9), 3, np.uint8), np.full((6, 9), 250, np.uint8), 8, 4, 62).any()


@pytest.mark.parametrize("name", ["gain", "gamma"])
def test_a_strictly_increasing_change_of_one_eye_leaves_the_volume_untouched(name):
    lut = cs.increasing_tables()[name]
    assert (np.diff(lut.astype(np.int64)) > 0).all()
    rng = np.random.default_rng(3)
    L, R = rng.integers(0, 128, (12, 40)).astype(np.uint8), rng.integers(0, 128, (12, 40)).astype(np.uint8)
    for r in (2, 4):
        assert np.array_equal(cs.census_volume(L, lut[R], 32, r, 62), cs.census_volume(L, R, 32, r, 62))
    # ... which the 1x3 SAD of the prefiltered images does not survive
    gL = cd.prefilter(L, 31)
    assert not np.array_equal(cd.sad3_volume(gL, cd.prefilter(lut[R], 31), 32), cd.sad3_volume(gL, cd.prefilter(R, 31), 32))


# ---- the ABI ----
def test_header_and_python_agree_on_the_constant(jn):
    from jackal_navigation_amd import sgm
    text = open(os.path.join(ROOT, "include", "jn_sgm_cost.h")).read()
    assert int(re.search(r"#define JN_SGM_COST_CENSUS\s+(\d+)", text).group(1)) == 4 == sgm.SGM_COST_CENSUS == cs.CENSUS
    assert C.sizeof(sgm.SgmCostParams) == 16
    assert "SELF-REFERENTIAL" in text and "UNTUNED" in text
    c = jn.Sgm.cost_parameters(cost_function=sgm.SGM_COST_CENSUS)               # the defaults make a valid 5x5 census whose clamp never bites
    assert (c.block_radius, c.cost_max) == (2, 127) and c.cost_max >= cs.bits(c.block_radius) and c.cost_max + jn.Sgm.parameters().P2 <= 255
    assert sorted(sgm.SGM_COST_EXPORTS) == ["jn_sgm_aggregate_batch", "jn_sgm_cost_params_default", "jn_sgm_cost_volume", "jn_sgm_create_cost"]
    assert jn.load().jn_version() == b"jn_stereo 0.4 (gfx950)"


def _status_codes():
    text = open(os.path.join(ROOT, "include", "jn_stereo.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(JN_[A-Z_]+)\s*=\s*(-?\d+)", text)}


BAD = [
    (dict(), dict(cost_function=cs.CENSUS, block_radius=1)), (dict(), dict(cost_function=cs.CENSUS, block_radius=5)),
    (dict(), dict(cost_function=cs.CENSUS, cost_max=0)), (dict(), dict(cost_function=cs.CENSUS, cost_max=196)),       # 196 + 60 = 256
    (dict(P2=200), dict(cost_function=cs.CENSUS, cost_max=56)),
    (dict(num_disparities=96), dict(cost_function=cs.CENSUS)), (dict(num_disparities=512), dict(cost_function=cs.CENSUS)),
    (dict(prefilter_cap=0), dict(cost_function=cs.CENSUS)), (dict(prefilter_cap=32), dict(cost_function=cs.CENSUS)),
    (dict(P1=-1), dict(cost_function=cs.CENSUS)), (dict(P1=61), dict(cost_function=cs.CENSUS)),
    (dict(), dict(cost_function=3)), (dict(), dict(cost_function=5)),
    (dict(), dict(cost_function=3, block_radius=4, cost_shift=0, cost_max=62)),
]


@pytest.mark.parametrize("pk,ck", BAD, ids=["%s-%s" % (sorted(a.items()), sorted(b.items())) for a, b in BAD])
def test_out_of_range_parameters_are_refused(jn, pk, ck):
    """Ahead of any device call, so also without a GPU."""
    from jackal_navigation_amd import sgm
    L = sgm._bind()
    h = C.c_void_p()
    p, c = jn.Sgm.parameters(**pk), jn.Sgm.cost_parameters(**ck)
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 1, 0, C.byref(h)) == _status_codes()["JN_ERR_UNSUPPORTED"]
    assert not h.value


GOOD = [dict(block_radius=2), dict(block_radius=3), dict(block_radius=4, cost_max=62), dict(cost_shift=12), dict(cost_shift=99), dict(cost_max=1),
        dict(cost_max=195)]


@pytest.mark.parametrize("ck", GOOD, ids=["%s" % sorted(a.items()) for a in GOOD])
def test_what_lies_inside_the_ranges_passes_the_range_checks(jn, ck):
    """cost_shift is ignored by the census cost.  With a GPU the handle is made, without one the call gets as far as the device."""
    from jackal_navigation_amd import sgm
    codes = _status_codes()
    L = sgm._bind()
    h = C.c_void_p()
    p, c = jn.Sgm.parameters(), jn.Sgm.cost_parameters(cost_function=sgm.SGM_COST_CENSUS, **ck)
    st = L.jn_sgm_create_cost(C.byref(p), C.byref(c), 64, 16, 1, 0, C.byref(h))
    assert st in (codes["JN_OK"], codes["JN_ERR_NO_DEVICE"])
    if st == codes["JN_OK"]:
        L.jn_sgm_destroy(h)
    else:
        assert not h.value


def test_invalid_arguments_stay_invalid(jn):
    from jackal_navigation_amd import sgm
    inv = _status_codes()["JN_ERR_INVALID"]
    L = sgm._bind()
    h = C.c_void_p()
    p, c = jn.Sgm.parameters(), jn.Sgm.cost_parameters(cost_function=sgm.SGM_COST_CENSUS)
    assert L.jn_sgm_create_cost(None, C.byref(c), 320, 180, 1, 0, C.byref(h)) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 1, 0, None) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 4, 180, 1, 0, C.byref(h)) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 0, 0, C.byref(h)) == inv


# ---- the kernels in the two builds ----
CENSUS_FAMILIES = ("k_census", "k_census_volume")
CENSUS_KERNELS = {"k_census<2, 2>", "k_census<3, 3>", "k_census<4, 3>"} | {"k_census_volume<%d, %s>" % (D, b) for D in (64, 128, 256) for b in ("true", "false")}


def census_instantiations(lib_path):
    """'k_name<args>' of the census kernels in a build of the library, from the host-side launch stubs (nm -C)."""
    out = subprocess.run(["nm", "-C", lib_path], capture_output=True, text=True, check=True).stdout
    return {name for name in re.findall(r"__device_stub__(\w+(?:<[^>]*>)?)\(", out) if name.split("<")[0] in CENSUS_FAMILIES}


def test_both_libraries_hold_every_census_kernel(jn):
    from jackal_navigation_amd import _lib
    assert census_instantiations(_lib.LIB_PATH) == CENSUS_KERNELS
    assert census_instantiations(_lib.HOOKS_LIB_PATH) == CENSUS_KERNELS
    assert not set(CENSUS_FAMILIES) & set(mc.MATCHER_FAMILIES)                 # the matcher matrix's two-sided check is about its own families

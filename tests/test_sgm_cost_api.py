"""The SGM mode over a cost volume (include/jn_sgm_cost.h): exports, struct layout, defaults, argument checking, and the anchors of its
scalar definition (tests/sgm_cost_def.py).  No GPU needed; the compute lives in tests/test_gpu_sgm_cost.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sgm_cost_def as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "jn_sgm_cost.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(jn_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_by_both_libraries(jn):
    from jackal_navigation_amd import sgm
    declared = _declared_functions()
    assert declared == sorted(sgm.SGM_COST_EXPORTS) == sorted(jn.SGM_COST_EXPORTS)
    assert len(declared) == 4
    assert not set(declared) & set(jn.SGM_EXPORTS)              # jn_sgm.h and SGM_EXPORTS stay what they were
    lib = jn.load()
    assert not [n for n in declared if not hasattr(lib, n)]
    with jn.hooks_library() as hooks:
        assert hooks is not lib
        assert not [n for n in declared if not hasattr(hooks, n)]
    for name in ("cost_volume", "aggregate", "cost_parameters"):
        assert hasattr(jn.Sgm, name), name


def test_version_is_unchanged(jn):
    assert jn.load().jn_version() == b"jn_stereo 0.4 (gfx950)"


def test_struct_layout_defaults_and_constants(jn):
    from jackal_navigation_amd import sgm
    P = sgm.SgmCostParams
    assert C.sizeof(P) == 16 and [f for f, _ in P._fields_] == ["cost_function", "block_radius", "cost_shift", "cost_max"]
    assert C.sizeof(sgm.SgmParams) == 24 and C.sizeof(sgm.SgmTimes) == 16      # no existing struct changed size
    c = jn.Sgm.cost_parameters()
    assert (c.cost_function, c.block_radius, c.cost_shift, c.cost_max) == (cd.BLOCK_SSD, 2, 5, 127)
    assert c.cost_max + jn.Sgm.parameters().P2 <= 255
    with pytest.raises(AttributeError):
        jn.Sgm.cost_parameters(radius=3)
    text = open(os.path.join(ROOT, "include", "jn_sgm_cost.h")).read()
    for name, v in (("SAD3", cd.SAD3), ("BLOCK_SSD", cd.BLOCK_SSD), ("EXTERNAL", cd.EXTERNAL)):
        assert int(re.search(r"#define JN_SGM_COST_%s\s+(\d+)" % name, text).group(1)) == v == getattr(sgm, "SGM_COST_" + name)
    assert "SELF-REFERENTIAL" in text


JN_ERR_INVALID, JN_ERR_UNSUPPORTED = -1, -4


def _status_codes():
    text = open(os.path.join(ROOT, "include", "jn_stereo.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(JN_[A-Z_]+)\s*=\s*(-?\d+)", text)}


BAD = [
    (dict(), dict(cost_function=3)), (dict(), dict(cost_function=-1)),
    (dict(), dict(block_radius=1)), (dict(), dict(block_radius=5)),
    (dict(), dict(cost_shift=-1)), (dict(), dict(cost_shift=13)),
    (dict(), dict(cost_max=0)), (dict(), dict(cost_max=196)), (dict(P2=129), dict()),
    (dict(num_disparities=96), dict()), (dict(num_disparities=32), dict()), (dict(num_disparities=512), dict()),
    (dict(prefilter_cap=0), dict()), (dict(prefilter_cap=32), dict()), (dict(P1=-1), dict()), (dict(P1=61), dict()),
    (dict(num_disparities=96), dict(cost_function=cd.EXTERNAL)), (dict(P2=255, P1=10), dict(cost_function=cd.EXTERNAL)),
    (dict(P2=250), dict(cost_function=cd.SAD3)),              # SAD3 is jn_sgm_create: 6 cap + P2 <= 255
]


@pytest.mark.parametrize("pk,ck", BAD, ids=["%s-%s" % (sorted(a.items()), sorted(b.items())) for a, b in BAD])
def test_out_of_range_parameters_are_refused(jn, pk, ck):
    """Ahead of any device call, so also without a GPU."""
    from jackal_navigation_amd import sgm
    codes = _status_codes()
    L = sgm._bind()
    h = C.c_void_p()
    p, c = jn.Sgm.parameters(**pk), jn.Sgm.cost_parameters(**ck)
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 1, 0, C.byref(h)) == codes["JN_ERR_UNSUPPORTED"]
    assert not h.value


def test_invalid_arguments(jn):
    from jackal_navigation_amd import sgm
    codes = _status_codes()
    L = sgm._bind()
    h = C.c_void_p()
    p, c = jn.Sgm.parameters(), jn.Sgm.cost_parameters()
    inv = codes["JN_ERR_INVALID"]
    assert L.jn_sgm_create_cost(None, C.byref(c), 320, 180, 1, 0, C.byref(h)) == inv
    assert L.jn_sgm_create_cost(C.byref(p), None, 320, 180, 1, 0, C.byref(h)) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 1, 0, None) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 4, 180, 1, 0, C.byref(h)) == inv
    assert L.jn_sgm_create_cost(C.byref(p), C.byref(c), 320, 180, 0, 0, C.byref(h)) == inv
    assert L.jn_sgm_cost_volume(None, 1, None, None, 0, 0, None) == inv
    assert L.jn_sgm_aggregate_batch(None, 1, None, None) == inv


# ---- the definition's anchors ----
CASES = [
    # W, H, D, seed, parameters
    (72, 40, 64, 1, dict()),
    (90, 33, 64, 2, dict(subpixel=1)),
    (70, 37, 64, 3, dict(lr_max_diff=-1, subpixel=1)),
    (50, 41, 64, 4, dict(P1=7, P2=100, prefilter_cap=20)),    # 3 P2 > 255: the "wide" three-path volume of the kernels
    (150, 24, 128, 5, dict(lr_max_diff=2, prefilter_cap=11)),
]


@pytest.mark.parametrize("W,H,D,seed,kw", CASES, ids=["%dx%d-D%d-%s" % (c[0], c[1], c[2], "+".join(sorted(c[4])) or "defaults") for c in CASES])
def test_aggregation_over_the_sad3_volume_equals_the_sgm_oracle(oracle, W, H, D, seed, kw):
    """jn_sgm.h's 1x3 SAD handed to the new definition's aggregation as its volume IS jn_sgm.h: bit for bit oracle/sgm_oracle.cpp."""
    from oracle.binding import SgmOracle
    sgm = SgmOracle()
    L, R = oracle.synth_pair(W, H, min(D - 16, 40), seed)
    p = sgm.params(num_disparities=D, **kw)
    want = sgm.process(p, L, R)
    gL, gR = cd.prefilter(L, p.prefilter_cap), cd.prefilter(R, p.prefilter_cap)
    assert np.array_equal(gL, sgm.prefilter(L, p.prefilter_cap)) and np.array_equal(gR, sgm.prefilter(R, p.prefilter_cap))
    got = cd.aggregate(cd.sad3_volume(gL, gR, D), p.P1, p.P2, p.lr_max_diff, p.subpixel)
    assert np.array_equal(got, want)
    assert (want >= 0).mean() > 0.3


def test_path_equals_the_sgm_oracles_single_path(oracle):
    from oracle.binding import SgmOracle
    sgm = SgmOracle()
    W, H, D = 60, 31, 64
    L, R = oracle.synth_pair(W, H, 30, 9)
    gL, gR = sgm.prefilter(L), sgm.prefilter(R)
    C_ = cd.sad3_volume(gL.astype(np.int64), gR.astype(np.int64), D)
    for dx, dy in cd.PATHS:
        assert np.array_equal(cd.path(C_, dx, dy, 10, 60), sgm.path(gL, gR, D, 10, 60, dx, dy).astype(np.int64)), (dx, dy)


@pytest.mark.parametrize("r", [2, 3, 4])
def test_ssd_equals_the_literal_triple_loop(r):
    rng = np.random.default_rng(r)
    W, H, D = 13, 9, 16                                        # narrower than D: every clamp is exercised
    gL, gR = rng.integers(0, 63, (H, W)).astype(np.int64), rng.integers(0, 63, (H, W)).astype(np.int64)
    assert np.array_equal(cd.ssd_volume(gL, gR, D, r), cd.ssd_literal(gL, gR, D, r))


def test_block_cost_clamps_and_shifts():
    rng = np.random.default_rng(0)
    L, R = rng.integers(0, 256, (20, 40)).astype(np.uint8), rng.integers(0, 256, (20, 40)).astype(np.uint8)
    ssd = cd.ssd_volume(cd.prefilter(L, 31), cd.prefilter(R, 31), 64, 2)
    c0 = cd.block_cost(L, R, 64, 31, 2, 0, 195)
    assert c0.dtype == np.uint8 and c0.max() == 195 and (c0 == 195).mean() > 0.9     # cost_shift = 0 saturates nearly everywhere
    c5 = cd.block_cost(L, R, 64, 31, 2, 5, 127)
    assert np.array_equal(c5, np.minimum(ssd // 32, 127)) and 0 < (c5 == 127).mean() < 1

"""The ELAS matrix without a GPU: tests/elas_cases.py launches every instantiation of the kernels of csrc/kernels.hip and csrc/delaunay_gpu.hip that
the release and the hooks library hold, names none they lack, every case is a valid call that gives the status it declares (by the CPU oracle),
and jn_elas_create's refusal at the limit of the key field sits where the restated arithmetic puts it."""
import os
import re

import numpy as np
import pytest

import elas_cases as ec
import elas_run
import matcher_cases as mc
from test_matcher_matrix import binary_instantiations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jackal_navigation_amd", "csrc")


def elas_families():
    """every __global__ of the two ELAS files: the node, tail, planner and matcher kernels live in files of their own"""
    names = set()
    for f in ("kernels.hip", "delaunay_gpu.hip"):
        names |= set(re.findall(r"__global__\s+void(?:\s+__launch_bounds__\(\w+\))?\s+(k_\w+)\s*\(", open(os.path.join(CSRC, f)).read()))
    assert len(names) >= 40 and not names & set(mc.MATCHER_FAMILIES), sorted(names)
    return names


def in_library(path):
    found = binary_instantiations(path, elas_families())
    return set().union(*found.values()), set(found)


def test_the_release_cases_launch_every_elas_kernel_in_the_release_library(jn):
    from jackal_navigation_amd import _lib
    binary, families = in_library(_lib.LIB_PATH)
    assert families == elas_families() - {"k_dt_dummy"}, "a kernel family is gone from the library (or nm's output changed): %s" % sorted(elas_families() - families)
    table = ec.table_instantiations(ec.RELEASE_CASES)
    assert not table - binary, "the dispatch restated in tests/elas_cases.py names kernels the release library does not hold: %s" % sorted(table - binary)
    assert binary - table == set(ec.UNREACHABLE_IN_RELEASE), "in the release library, launched by no release case of tests/elas_cases.py: %s" % sorted(binary - table)
    # the set may not grow silently
    assert sorted(ec.UNREACHABLE_IN_RELEASE) == ["k_support"] and all(len(r) > 20 for r in ec.UNREACHABLE_IN_RELEASE.values())


def test_the_hooks_cases_launch_what_is_left_in_the_hooks_library(jn):
    from jackal_navigation_amd import _lib
    binary, families = in_library(_lib.HOOKS_LIB_PATH)
    assert families == elas_families()
    table = ec.table_instantiations(ec.ALL_CASES)
    assert not binary - table, "in the hooks library, launched by no case: %s" % sorted(binary - table)
    assert not table - binary, "the restated dispatch names kernels the hooks library does not hold: %s" % sorted(table - binary)
    hooks_only = ec.table_instantiations(ec.HOOKS_CASES)
    assert set(ec.UNREACHABLE_IN_RELEASE) <= hooks_only, "what the release library cannot reach must run in a hooks case"
    assert "k_dt_dummy" in hooks_only


def test_the_table_says_which_case_covers_which_form():
    """the parameter-driven forms by name: the four support buckets in both flows and with 1, 2, 3 and 8 segments, both dense forms ..."""
    routes = {(ec.support_route(c), ec.plane_flow(c)) for c in ec.ALL_CASES}
    assert {(r[0], plane) for r, plane in routes if r} == {(b, f) for b in (320, 640, 1280, 2560) for f in (False, True)}
    assert {r[1] for r, _ in routes if r} >= {1, 2, 3, 5, 8} and (None, False) in routes and (None, True) not in routes
    assert {ec.filter_form(c) for c in ec.RELEASE_CASES} == {0, 1, 2}
    covered = {}
    for c in ec.ALL_CASES:
        for k in ec.elas_instantiations(c):
            covered.setdefault(k, []).append(ec.case_id(c))
    for k in ("k_dense_row<4>", "k_dense_row<8>", "k_dense", "k_bin<true>", "k_bin<false>", "k_tri_setup", "k_gap<true>", "k_gap4<true>", "k_gap_rows_any", "k_adaptive_mean_h",
              "k_adaptive_mean_h4", "k_copy_ok", "k_lr", "k_grid_mark", "k_arrange<0>", "k_arrange<2>", "k_delaunay_sub<true>", "k_support_filters<5, 8>"):
        assert len(covered.get(k, [])) >= 1, k
    # an odd number of pixels never reaches launch_copy_ok: the fused pass that calls it asks for W * H % 4 == 0
    odd = [c for c in ec.RELEASE_CASES if (c.W * c.H) & 3 and not c.kw.get("postprocess_only_left", 1) and not c.kw.get("subsampling")]
    assert odd and all("k_copy_ok" not in ec.elas_instantiations(c) and "k_gap_mean_fused" not in ec.elas_instantiations(c) for c in odd)


def test_case_ids_are_unique_and_every_child_has_cases():
    ids = [ec.case_id(c) for c in ec.ALL_CASES]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    assert all(" " not in i for i in ids)                                  # they travel on a command line
    assert {c.run["child"] for c in ec.ALL_CASES if c.run.get("child")} | {"sgm_tail3"} == set(ec.CHILDREN)
    for c in ec.ALL_CASES:
        assert c.hooks == any(k in c.env for k in HOOK_NAMES) or c.run.get("child"), (ec.case_id(c), "takes the hooks build exactly when it sets one of its knobs")
        assert c in ec.HOOKS_CASES if c.hooks else c in ec.RELEASE_CASES


HOOK_NAMES = ("JN_SUPPORT_SPLIT", "JN_SUPPORT_SEGMENTS", "JN_FUSE_LIST", "JN_BIN_SETUP", "JN_DENSE_XCD_ORDER", "JN_POST_BAND", "JN_ARRANGE_GLOBAL", "JN_DT_DUMMY", "JN_DT_DUMMY_US",
              "JN_FILTER_LDS_KB")


def test_hook_names_are_the_hooks_builds(jn):
    """what the table treats as a hooks-only knob is read through JN_HOOK_ENV, what it treats as shipped through getenv"""
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("kernels.hip", "jn_api.cpp", "elas_api.cpp", "elas_batch.cpp", "elas_seams.cpp", "delaunay_gpu.hip"))
    used = {k for c in ec.ALL_CASES for k in c.env}
    for k in used:
        hook, shipped = 'JN_HOOK_ENV("%s")' % k in src, 'getenv("%s")' % k in src.replace("JN_HOOK_ENV(", "hook(")
        assert hook != shipped and hook == (k in HOOK_NAMES), k


def test_every_case_is_a_valid_call():
    for c in ec.ALL_CASES:
        assert ec.create_status(c) == 0, ec.case_id(c)
        assert 1 <= c.run["host_threads"] < 14 and c.flow in ("plane", "desc") and ec.plane_flow(c) == (c.flow == "plane"), ec.case_id(c)
        assert not c.kw.get("subsampling") or c.n == 1                     # (the runner compares half-size maps of a lone pair only)
        assert c.W * c.H <= 2600 * 64                                      # small frames: the suite has 720p and 1080p on the default route


@pytest.mark.parametrize("c", ec.ALL_CASES, ids=[ec.case_id(c) for c in ec.ALL_CASES])
def test_case_status_on_the_cpu(oracle, c):
    """every frame finds its support points (status 0) except the noise frame a case declares: a frame too small or too flat for the lattice
    would make the GPU test compare untouched buffers; and the map has content (1000 valid pixels: more than any one tile, strip or band holds)"""
    Ls, Rs = ec.images(c, oracle)
    st, D1, D2 = elas_run.expected(oracle, c, Ls, Rs)
    assert st == [1 if b == c.run.get("noise") else 0 for b in range(c.n)], (ec.case_id(c), c.why)
    for b in range(c.n):
        if st[b] == 0:
            px = D1[b].size // 4 if c.kw.get("subsampling") else D1[b].size
            valid = D1[b].reshape(-1)[:px] >= 0
            assert not (D1[b].reshape(-1)[:px] == elas_run.FILL).any() and valid.sum() >= 1000, (ec.case_id(c), b, int(valid.sum()))


def test_prior_limit_edges():
    """|P[0]| just below 2^19 is accepted, just above is JN_ERR_UNSUPPORTED, by the restated float arithmetic (jn_elas_create looks at the priors after it
    has found its device: tests/test_gpu_elas_matrix.py asks the library itself)"""
    ok, refused = ec.prior_edge_betas()
    p_ok, p_no = ec.priors(dict(ec.DEFAULTS, beta=ok)), ec.priors(dict(ec.DEFAULTS, beta=refused))
    assert ec.PRIOR_LIMIT * 0.9995 < -p_ok[0] < ec.PRIOR_LIMIT < -p_no[0] < ec.PRIOR_LIMIT * 1.0005 and 5.4e-7 < refused < ok < 5.6e-7
    assert max(abs(v) for v in p_ok) == -p_ok[0]
    mk = lambda **kw: ec.case(160, 120, 30, 63, 7, 1, kw, "")
    assert ec.create_status(mk(beta=refused)) == 2 and ec.create_status(mk(beta=ok)) == 0
    # the other fall-back triggers, as restated
    assert not ec.dense_row_applies(mk(beta=3e-5)) and ec.dense_row_applies(mk(beta=4e-5)) and max(abs(v) for v in ec.priors(dict(ec.DEFAULTS, beta=3e-5))) > 8000
    assert not ec.dense_row_applies(mk(grid_size=7)) and ec.dense_row_applies(mk(grid_size=8))

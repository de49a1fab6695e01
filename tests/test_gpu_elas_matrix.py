"""Every route of the ELAS path against the CPU oracle, bit for bit: the cases of tests/elas_cases.py (the fall-back flow with materialised descriptors
as the parameters and JN_DESC_FLOW choose it, the shipped switches, the hooks build's route-forcing knobs, the parameter-driven kernel forms), each
with the flow it expects asserted through jn_elas_route_stats.  Switches that a launcher reads once per process run in fresh child processes
(tests/mocks/elas_route_worker.py), one after the other."""
import ctypes as C
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

import elas_cases as ec
import elas_run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mocks", "elas_route_worker.py")
IN_PROCESS = [c for c in ec.ALL_CASES if not c.run.get("child")]


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's answer of a case, computed once per distinct (frame, parameters): many cases differ in their switches only"""
    memo = {}

    def get(c):
        key = (c.W, c.H, c.sd, c.disp_max, c.seed, c.n, tuple(sorted(c.kw.items())), c.run.get("noise"))
        if key not in memo:
            Ls, Rs = ec.images(c, oracle)
            memo[key] = (Ls, Rs) + elas_run.expected(oracle, c, Ls, Rs)
            for a in memo[key][:2] + memo[key][3:]:
                a.setflags(write=False)
        return memo[key]
    return get


def check_route(c, stats):
    assert stats[2] == (1 if c.flow == "plane" else 0), "%s [%s]: jn_elas_route_stats says the %s flow ran" % (ec.case_id(c), c.why, "plane" if stats[2] else "descriptor")
    assert stats[0] == (1 if c.run.get("gpu_dt") else 0), "%s [%s]: GPU triangulation %d" % (ec.case_id(c), c.why, stats[0])
    assert stats[1] == 0, "%s [%s]: the GPU triangulation handed the batch back to the host" % (ec.case_id(c), c.why)


@pytest.mark.parametrize("c", IN_PROCESS, ids=[("hooks-" if c.hooks else "") + ec.case_id(c) for c in IN_PROCESS])
def test_elas_case(jn, same, want, monkeypatch, c):
    for k in [k for k in os.environ if k.startswith("JN_") and k not in ("JN_STEREO_LIB", "JN_RCCL_LIB")]:
        monkeypatch.delenv(k)
    for k, v in ec.effective_env(c).items():
        monkeypatch.setenv(k, v)
    Ls, Rs, st_o, D1o, D2o = want(c)
    if c.hooks:
        with jn.hooks_library():
            st, outs, stats = elas_run.run_case(jn, c, Ls, Rs)
    else:
        st, outs, stats = elas_run.run_case(jn, c, Ls, Rs)
    check_route(c, stats)
    assert st == st_o, (ec.case_id(c), c.why)
    for s, (D1, D2) in enumerate(outs):
        for b in range(c.n):
            assert same(D1[b], D1o[b]), "%s [%s]: slot %d frame %d, %d pixels of D1 differ" % (ec.case_id(c), c.why, s, b, int((D1[b] != D1o[b]).sum()))
            assert same(D2[b], D2o[b]), "%s [%s]: slot %d frame %d, %d pixels of D2 differ" % (ec.case_id(c), c.why, s, b, int((D2[b] != D2o[b]).sum()))
    if "noise" in c.run:
        assert (outs[0][0][c.run["noise"]] == elas_run.FILL).all() and st[c.run["noise"]] == 1


def test_create_refuses_a_prior_beyond_the_key_field(jn):
    """|P[0]| just above 2^19: JN_ERR_UNSUPPORTED (the accepted side of the edge is a case of the table)"""
    from jackal_navigation_amd import _lib
    ok, refused = ec.prior_edge_betas()
    h = C.c_void_p()
    assert jn.load().jn_elas_create(C.byref(jn.Elas.parameters(0, disp_max=63, beta=refused)), 160, 120, 1, 0, 1, 1, C.byref(h)) == _lib.JN_ERR_UNSUPPORTED
    assert any(c.kw.get("beta") == ok and c.n == 1 for c in ec.RELEASE_CASES) and any(c.kw.get("beta") == ok and c.n == 3 for c in ec.RELEASE_CASES)


# seconds from a child's start to its exit (import, HIP start-up and its cases), measured on an MI355X with the libraries of the parent commit; the
# time-out of a child is five times that, for a busy shared machine
CHILD_SECONDS = {"lr_ccl_split": 2.25, "grid_late": 2.15, "wavefront": 2.22, "sgm_tail3": 2.22, "hooks_a": 2.14, "hooks_b": 2.23, "hooks_c": 2.33}


def test_once_per_process_switches_in_fresh_children(jn, oracle, want):
    """JN_LR_CCL_FUSED=0, JN_GRID_EARLY=0, JN_FILTER_WAVEFRONT=1, JN_SGM_TAIL=3 and the hooks build's static knobs (JN_SUPPORT_SEGMENTS, JN_FUSE_LIST,
    JN_BIN_SETUP, JN_DENSE_XCD_ORDER, JN_POST_BAND, JN_DT_DUMMY) are read once per process: one fresh child each (elas_cases.CHILDREN), strictly one
    after the other; the first child that times out, dies of a signal or exits non-zero ends the test.  Measured start-to-exit times of the children: 2.1 to
    2.4 s each (CHILD_SECONDS; a child's time-out is five times its own), 15.5 s for the seven."""
    from jackal_navigation_amd import _lib
    from oracle.binding import SgmOracle
    assert set(CHILD_SECONDS) == set(ec.CHILDREN)
    for name, (hooks, env_c) in ec.CHILDREN.items():
        cases = [c for c in ec.ALL_CASES if c.run.get("child") == name]
        ids = [ec.case_id(c) for c in cases] + ([ec.SGM_TAIL_ID] if name == "sgm_tail3" else [])
        env = {k: v for k, v in os.environ.items() if not k.startswith("JN_") or k == "JN_RCCL_LIB"}
        env.update(ec.BASE_ENV)
        env.update(env_c)
        if hooks:
            env["JN_STEREO_LIB"] = _lib.HOOKS_LIB_PATH
        r = subprocess.run([sys.executable, WORKER] + ids, env=env, capture_output=True, text=True, timeout=5 * CHILD_SECONDS[name])
        assert r.returncode == 0, "child %s: %s\n%s" % (name, "signal %s" % signal.Signals(-r.returncode).name if r.returncode < 0 else "exit %d" % r.returncode,
                                                      r.stderr[-2000:])
        lines = [l for l in r.stdout.splitlines() if l.startswith("ELAS_ROUTE_WORKER ")]
        assert len(lines) == 1, r.stdout[-2000:]
        got = json.loads(lines[0][len("ELAS_ROUTE_WORKER "):])
        assert sorted(got) == sorted(ids)
        for c in cases:
            g = got[ec.case_id(c)]
            _, _, st_o, D1o, D2o = want(c)
            check_route(c, g["route"])
            assert g["status"] == st_o and len(g["d1"]) == c.run["slots"], (name, ec.case_id(c))
            for h1, h2 in zip(g["d1"], g["d2"]):
                assert int(h1, 16) == oracle.fnv(D1o) and int(h2, 16) == oracle.fnv(D2o), "child %s, %s [%s]: D1 / D2 differ from the oracle's" % (name, ec.case_id(c), c.why)
        if name == "sgm_tail3":
            g = got[ec.SGM_TAIL_ID]
            assert g["scan"] == g["sync"], "jn_sgm_submit_scan under JN_SGM_TAIL=3: map, u8 map or bins differ from the synchronous three-call route's"
            W, H, D, n = ec.SGM_TAIL_FRAME
            sgm = SgmOracle()
            pairs = [oracle.synth_pair(W, H, 40, 700 + b) for b in range(n)]
            exp = np.ascontiguousarray(np.stack([sgm.process(sgm.params(D), L, R) for L, R in pairs]), np.int16)
            assert int(g["scan"][0], 16) == oracle.fnv(exp.view(np.uint32)), "the map under JN_SGM_TAIL=3 differs from the SGM oracle's"

"""One fresh process of tests/test_gpu_elas_matrix.py (TEST INFRASTRUCTURE): the switches that a launcher reads once per process
(JN_LR_CCL_FUSED, JN_GRID_EARLY, JN_FILTER_WAVEFRONT, JN_SGM_TAIL, the hooks build's static knobs) cannot be flipped inside pytest.
    python elas_route_worker.py <case id> ...      ids of tests/elas_cases.py, or elas_cases.SGM_TAIL_ID
The environment (the switches, JN_STEREO_LIB for the hooks build) comes from the parent.  Runs every case through the package and prints one line
"ELAS_ROUTE_WORKER <json>": per id the frames' status, the FNV hash (jn_fnv1a64_u32) of D1 and D2 of every slot and jn_elas_route_stats.  The parent
compares them with the oracle's."""
import ctypes as C
import json
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]


def fnv(lib, a):
    a = np.ascontiguousarray(a)
    assert a.nbytes % 4 == 0
    lib.jn_fnv1a64_u32.restype = C.c_uint64
    return "%016x" % lib.jn_fnv1a64_u32(a.ctypes.data_as(C.c_void_p), C.c_int64(a.nbytes // 4))


def sgm_tail(jn, lib):
    """jn_sgm_submit_scan (under JN_SGM_TAIL=3: three kernels behind the sweeps) and the synchronous three-call route on the same frames"""
    import elas_cases as ec
    from jackal_navigation_amd import node
    from jackal_navigation_amd.device import DeviceArray
    from oracle.binding import Oracle
    W, H, D, n = ec.SGM_TAIL_FRAME
    o = Oracle()
    pairs = [o.synth_pair(W, H, 40, 700 + b) for b in range(n)]
    Ls, Rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    new = lambda: (DeviceArray((n, H, W), np.int16), DeviceArray((n, H, W), np.uint8), DeviceArray((n, sp.bins), np.float64), DeviceArray((n, 4), np.float64))
    with jn.Sgm(jn.Sgm.parameters(num_disparities=D), W, H, max_batch=n) as m:
        dd, du, bins, meta = new()
        m.process_batch(n, dL.ptr, dR.ptr, W, H * W, dd.ptr)
        m.to_u8(dd.ptr, du.ptr, n * H * W)
        node.obstacle_scan(sp, n, du.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
        sync = [a.numpy().copy() for a in (dd, du, bins)]
        qd, qu, qb, qm = new()
        m.submit_scan(0, n, dL.ptr, dR.ptr, W, H * W, qd.ptr, sp, lut.ptr, qu.ptr, qb.ptr, qm.ptr)
        m.wait(0)
        scan = [a.numpy().copy() for a in (qd, qu, qb)]
    return {"sync": [fnv(lib, a) for a in sync], "scan": [fnv(lib, a) for a in scan]}


def main():
    import elas_cases as ec
    import elas_run
    import jackal_navigation_amd as jn
    from oracle.binding import Oracle
    lib = jn.load()
    o = Oracle()
    out = {}
    for cid in sys.argv[1:]:
        if cid == ec.SGM_TAIL_ID:
            out[cid] = sgm_tail(jn, lib)
            continue
        c = ec.BY_ID[cid]
        for k, v in ec.CHILDREN[c.run["child"]][1].items():
            assert os.environ.get(k) == v, "the parent did not pass %s=%s" % (k, v)
        os.environ.update(ec.effective_env(c))                   # what is left is read per handle or per batch
        Ls, Rs = ec.images(c, o)
        st, outs, stats = elas_run.run_case(jn, c, Ls, Rs)
        out[cid] = {"status": [int(s) for s in st], "d1": [fnv(lib, d1) for d1, _ in outs], "d2": [fnv(lib, d2) for _, d2 in outs], "route": list(stats)}
    sys.stdout.flush()
    print("ELAS_ROUTE_WORKER " + json.dumps(out), flush=True)


main()

"""Every kernel form of the SGM and block-matching modes against its scalar definition (oracle/sgm_oracle.cpp, oracle/bm_oracle.cpp; still
self-referential: the reference has neither matcher), at the parameter edges of tests/matcher_cases.py, through the C ABI of the release library."""
import ctypes as C

import numpy as np
import pytest

import matcher_cases as mc
from matcher_run import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sgm():
    from oracle.binding import SgmOracle
    return SgmOracle()


@pytest.fixture(scope="module")
def bm():
    from oracle.binding import BmOracle
    return BmOracle()


def same_map(c, what, got, exp):
    bad = np.argwhere(got != exp)
    assert not len(bad), "%s [%s] %s: %d of %d pixels differ, first (y, x) %s: got %s, expected %s" % (
        mc.case_id(c), c.why, what, len(bad), exp.size, bad[:5].tolist(), [int(got[tuple(i)]) for i in bad[:5]], [int(exp[tuple(i)]) for i in bad[:5]])


def check_sgm_case(jn, sgm, oracle, c):
    Ls, Rs = mc.images(c, oracle)
    if c.edge:
        m, _, top = mc.path_excess(sgm, Ls[0], Rs[0], c.D, c.kw)
        assert not mc.sgm_edges(c, m, top), "%s [%s]: the images do not reach %s" % (mc.case_id(c), c.why, mc.sgm_edges(c, m, top))
    out, u8, _ = run(jn, jn.Sgm, jn.Sgm.parameters(num_disparities=c.D, **c.kw), Ls, Rs, **c.layout)
    po = sgm.params(c.D, **c.kw)
    for b in range(c.n):
        exp = sgm.process(po, Ls[b], Rs[b])
        same_map(c, "frame %d" % b, out[b], exp)
        same_map(c, "u8 map of frame %d" % b, u8[b], sgm.to_u8(exp, c.kw.get("subpixel", 0)))


@pytest.mark.parametrize("c", mc.SGM_CASES, ids=[mc.case_id(c) for c in mc.SGM_CASES])
def test_sgm_case(jn, sgm, oracle, c):
    check_sgm_case(jn, sgm, oracle, c)


@pytest.mark.parametrize("env,c", mc.SGM_HOOKS_CASES, ids=["%s-%s" % ("".join("%s%s" % kv for kv in env.items()), mc.case_id(c)) for env, c in mc.SGM_HOOKS_CASES])
def test_sgm_forms_of_the_hooks_build(jn, hooks, sgm, oracle, monkeypatch, env, c):
    """2 and 8 strips per workgroup, four lanes per pixel at D = 256: what the evidence runs' A/B lines time (JN_SGM_NS, JN_SGM_LQ)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    check_sgm_case(jn, sgm, oracle, c)


@pytest.mark.parametrize("c", mc.BM_CASES, ids=[("ssd-" if c.kw.get("cost_function") else "sad-") + mc.case_id(c) for c in mc.BM_CASES])
def test_bm_case(jn, bm, sgm, oracle, c):
    Ls, Rs = mc.images(c, oracle)
    out, u8, _ = run(jn, jn.Bm, jn.Bm.parameters(num_disparities=c.D, **c.kw), Ls, Rs, **c.layout)
    po = bm.params(c.D, **c.kw)
    for b in range(c.n):
        exp = bm.process(po, Ls[b], Rs[b])
        same_map(c, "frame %d" % b, out[b], exp)
        same_map(c, "u8 map of frame %d" % b, u8[b], sgm.to_u8(exp, c.kw.get("subpixel", 0)))
    if c.scene == "peak":
        assert (out[0][:, 17:] >= 0).all() and len(np.unique(out[0][:, 17:])) > 8          # the lone zero-cost candidate moves with x


WIDE_CASES = [c for c in mc.SGM_CASES if "wide" in c.edge]


@pytest.mark.parametrize("c", WIDE_CASES, ids=[mc.case_id(c) for c in WIDE_CASES])
def test_sgm_wide_cases_through_the_pipelined_form(jn, sgm, oracle, c):
    """jn_sgm_submit_scan with scan parameters on slots 0 and 1 (slot 1 allocates its own doubled three-path volume; the fused tail reads the
    winners) against the synchronous three-call route and the oracle chain"""
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node
    W, H, n = c.W, c.H, c.n
    Ls, Rs = mc.images(c, oracle)
    sp, spo = node.scan_params(W, H), oracle.scan_params(W, H)
    lut, luto = node.build_valid_disp_lut(sp, W, H), oracle.valid_lut(spo, W, H)
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    new = lambda: (DeviceArray((n, H, W), np.int16), DeviceArray((n, H, W), np.uint8), DeviceArray((n, sp.bins), np.float64), DeviceArray((n, 4), np.float64))
    with jn.Sgm(jn.Sgm.parameters(num_disparities=c.D, **c.kw), W, H, max_batch=n) as m:
        dd, du, bins, meta = new()
        m.process_batch(n, dL.ptr, dR.ptr, W, H * W, dd.ptr)
        m.to_u8(dd.ptr, du.ptr, n * H * W)
        node.obstacle_scan(sp, n, du.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
        want = [a.numpy().copy() for a in (dd, du, bins, meta)]
        outs = [new(), new()]
        for slot in (0, 1):
            m.submit_scan(slot, n, dL.ptr, dR.ptr, W, H * W, outs[slot][0].ptr, sp, lut.ptr, outs[slot][1].ptr, outs[slot][2].ptr, outs[slot][3].ptr)
        for slot in (0, 1):
            m.wait(slot)
            for name, a, b in zip(("disparities", "u8 map", "bins", "meta"), want, outs[slot]):
                assert np.array_equal(a, b.numpy()), "%s [%s]: slot %d's %s differ from the synchronous route's" % (mc.case_id(c), c.why, slot, name)
    po = sgm.params(c.D, **c.kw)
    for b in range(n):
        exp = sgm.process(po, Ls[b], Rs[b])
        u8o = sgm.to_u8(exp, c.kw.get("subpixel", 0))
        same_map(c, "frame %d" % b, want[0][b], exp)
        same_map(c, "u8 map of frame %d" % b, want[1][b], u8o)
        bo, mo, _ = oracle.scan(spo, u8o, luto)
        assert np.allclose(want[2][b], bo, rtol=0, atol=1e-4) and np.allclose(want[3][b], mo, rtol=0, atol=1e-4), (mc.case_id(c), b)


STAGE_CASES = [c for c in mc.SGM_CASES if c.edge in (("top", "byte"), ("top", "wide")) and c.kw.get("P2") in (69, 86)]


@pytest.mark.parametrize("c", STAGE_CASES, ids=[mc.case_id(c) for c in STAGE_CASES])
def test_sgm_volumes_stage_by_stage(jn, sgm, oracle, c):
    """The two horizontal volumes and the downward three-path volume (jn_sgm_debug_ptr) against sums of the oracle's paths minus the cost: the
    volumes hold P2 - (L_r - C) per path, columns mirrored, a pixel's disparities in the kernels' own order.  Says WHICH sweep is wrong."""
    from jackal_navigation_amd import _lib
    from jackal_navigation_amd.device import DeviceArray
    assert len(STAGE_CASES) == 6
    Ls, Rs = mc.images(c, oracle)
    n, H, W, D = c.n, c.H, c.W, c.D
    dL, dR, dD = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs), DeviceArray((n, H, W), np.int16)

    def d2h(ptr, dtype):
        out = np.empty((n, H, W, D), dtype)
        _lib.check(_lib.load().jn_memcpy_d2h(0, out.ctypes.data_as(C.c_void_p), ptr, out.nbytes), "jn_memcpy_d2h")
        return out.astype(np.int32)

    with jn.Sgm(jn.Sgm.parameters(num_disparities=D, **c.kw), W, H, max_batch=n) as s:
        s.process_batch(n, dL.ptr, dR.ptr, W, H * W, dD.ptr)
        ptr, info = s.debug_ptr(0)
        wide = info[0]
        assert wide == (1 if "wide" in c.edge else 0)
        vF = d2h(ptr, np.uint16 if wide else np.uint8)
        vH0, vH1 = d2h(s.debug_ptr(1)[0], np.uint8), d2h(s.debug_ptr(2)[0], np.uint8)
    P2 = c.kw["P2"]
    ob, of = mc.volume_order(D, 0), mc.volume_order(D, wide)
    for b in range(n):
        m, _, _ = mc.path_excess(sgm, Ls[b], Rs[b], D, c.kw)
        same_map(c, "frame %d, horizontal volume of the path (-1, 0)" % b, vH0[b], (P2 - m[(-1, 0)])[:, ::-1][:, :, ob])
        same_map(c, "frame %d, horizontal volume of the path (+1, 0)" % b, vH1[b], (P2 - m[(1, 0)])[:, ::-1][:, :, ob])
        same_map(c, "frame %d, three-path volume of the downward sweep" % b, vF[b], (3 * P2 - sum(m[d] for d in mc.DOWN))[:, ::-1][:, :, of])
    for a in (dL, dR, dD):
        a.free()


@pytest.mark.parametrize("subpixel", [0, 1])
def test_disparity_to_u8_on_every_int16(jn, sgm, subpixel):
    from jackal_navigation_amd.device import DeviceArray
    v = np.arange(-32768, 32768, dtype=np.int16)
    dV, dU = DeviceArray.from_numpy(v), DeviceArray((v.size,), np.uint8)
    with jn.Sgm(jn.Sgm.parameters(num_disparities=64, subpixel=subpixel), 8, 8) as s:
        s.to_u8(dV.ptr, dU.ptr, v.size)
    got = dU.numpy()
    assert np.array_equal(got, sgm.to_u8(v, subpixel))
    w = v.astype(np.int64)
    q = np.rint(w / 16.0) if subpixel else w                        # numpy rounds halves to even; sixteenths are exact in binary
    assert np.array_equal(got, np.where(w < 0, 0, np.minimum(q, 255)).astype(np.uint8))
    for a in (dV, dU):
        a.free()

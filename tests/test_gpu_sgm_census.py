"""The census / Hamming cost of the SGM mode (include/jn_sgm_cost.h, JN_SGM_COST_CENSUS) on the GPU, bit for bit against its definition
(tests/sgm_census_def.py): the producer (k_census, k_census_volume), the handle end to end, producer + an external consumer, the
pipelined slots with the scan tail, the invariance the mode exists for, and the other costs next to it in one process."""
import numpy as np
import pytest

import matcher_cases as mc
import scenes
import sgm_census_def as cs
import sgm_cost_def as cd
from matcher_run import run, LEFT_POISON, RIGHT_POISON

pytestmark = pytest.mark.gpu

GUARD = 4096                                                   # bytes either side of a caller's volume that must come back untouched


def _dev(jn):
    from jackal_navigation_amd.device import DeviceArray
    return DeviceArray


def _census(jn, **kw):
    from jackal_navigation_amd import sgm
    return jn.Sgm.cost_parameters(cost_function=sgm.SGM_COST_CENSUS, **kw)


def _pair(oracle, scene, W, H, seed):
    if scene == "synth":
        return oracle.synth_pair(W, H, 40, seed)
    if scene in scenes.KINDS:
        return scenes.make_scene(scene, W, H, 40, seed)
    return mc.PAIRS[scene](W, H, seed)


def _volume(jn, pairs, D, r, cmax, P2=60, extra=0, pad=0, gap=0):
    """jn_sgm_cost_volume of a census handle into a buffer with guard bytes either side -> [n][H][W][D]"""
    DeviceArray = _dev(jn)
    n = len(pairs)
    H, W = pairs[0][0].shape
    pitch, rows = W + pad, H + gap
    Lp = np.full((n, rows, pitch), LEFT_POISON, np.uint8); Rp = np.full((n, rows, pitch), RIGHT_POISON, np.uint8)
    for b, (L, R) in enumerate(pairs):
        Lp[b, :H, :W] = L; Rp[b, :H, :W] = R
    dL, dR = DeviceArray.from_numpy(Lp), DeviceArray.from_numpy(Rp)
    size = n * H * W * D
    dC = DeviceArray.from_numpy(np.full(size + 2 * GUARD, 0xEE, np.uint8))
    p = jn.Sgm.parameters(num_disparities=D, P2=P2)
    with jn.Sgm(p, W, H, max_batch=n + extra, cost=_census(jn, block_radius=r, cost_max=cmax)) as m:
        m.cost_volume(n, dL.ptr, dR.ptr, pitch, rows * pitch, dC.ptr + GUARD)
    buf = dC.numpy()
    assert (buf[:GUARD] == 0xEE).all() and (buf[GUARD + size:] == 0xEE).all(), "the producer wrote outside the volume"
    for a in (dL, dR, dC):
        a.free()
    return buf[GUARD:GUARD + size].reshape(n, H, W, D)


VOLUME_CASES = [
    # W, H, D, r, cost_max, P2, scene, n, extra, pad, gap
    (200, 50, 64, 2, 127, 60, "synth", 1, 0, 0, 0),
    (70, 33, 64, 3, 127, 60, "grain", 1, 0, 0, 0),
    (333, 21, 64, 4, 62, 60, "synth", 1, 0, 0, 0),               # more than one tile of 256 columns, the last one partly filled
    (150, 41, 128, 2, 24, 60, "strips", 2, 0, 0, 0),
    (133, 29, 128, 3, 9, 60, "synth", 1, 0, 0, 0),               # a cost_max that clamps
    (333, 19, 128, 4, 127, 60, "photometric", 1, 0, 0, 0),
    (100, 37, 256, 2, 5, 60, "synth", 1, 0, 0, 0),               # a frame narrower than D; clamps
    (70, 27, 256, 3, 48, 60, "noise", 1, 0, 0, 0),
    (300, 17, 256, 4, 61, 60, "noise", 1, 0, 0, 0),              # one below the window's bits: the clamp bites at the very top only
    (40, 8, 128, 4, 127, 60, "noise", 2, 0, 0, 0),               # H = 8: the 9x7 window is nearly as high as the image
    (8, 8, 64, 4, 127, 60, "noise", 1, 0, 0, 0),                 # the smallest frame: the window is wider and as high as the image
    (157, 43, 64, 3, 30, 100, "synth", 2, 1, 5, 3),              # odd pitch, gap rows, n < max_batch
    (261, 30, 128, 4, 127, 60, "blobs", 3, 0, 13, 2),
]


@pytest.mark.parametrize("W,H,D,r,cmax,P2,scene,n,extra,pad,gap", VOLUME_CASES,
                         ids=["%dx%d-D%d-r%d-m%d-%s" % (c[0], c[1], c[2], c[3], c[4], c[6]) for c in VOLUME_CASES])
def test_cost_volume_equals_the_definition(jn, oracle, W, H, D, r, cmax, P2, scene, n, extra, pad, gap):
    pairs = [_pair(oracle, scene, W, H, 70 + b) for b in range(n)]
    got = _volume(jn, pairs, D, r, cmax, P2, extra, pad, gap)
    for b, (L, R) in enumerate(pairs):
        assert np.array_equal(got[b], cs.census_volume(L, R, D, r, cmax)), b
    if cmax < cs.bits(r):
        assert (got == cmax).any(), "the case is meant to clamp"


@pytest.mark.parametrize("r", [2, 3, 4])
def test_constant_images_and_step_edges_at_the_borders(jn, r):
    W, H, D = 90, 20, 64
    flatL, flatR = np.full((H, W), 17, np.uint8), np.full((H, W), 230, np.uint8)
    assert not _volume(jn, [(flatL, flatR)], D, r, 127).any()                 # every signature is empty, whatever the two grey levels
    for col in (0, W - 1):                                                     # a vertical step edge in the first / last column: the clamps
        L = np.full((H, W), 100, np.uint8); L[:, col] = 20
        R = np.full((H, W), 100, np.uint8); R[:, col] = 180
        got = _volume(jn, [(L, R)], D, r, 127)[0]
        assert np.array_equal(got, cs.census_volume(L, R, D, r, 127))
        assert got.any()


E2E_CASES = [
    # W, H, D, r, cost_max, parameters
    (170, 48, 64, 2, 127, dict()),
    (203, 41, 128, 3, 127, dict(subpixel=1)),
    (140, 36, 256, 4, 62, dict(subpixel=1, lr_max_diff=1)),
    (150, 40, 128, 4, 40, dict(lr_max_diff=-1, P1=20, P2=120)),   # a clamp, no L/R check, the P2 other libraries pair with 9x7 ("wide")
    (90, 44, 64, 2, 20, dict(P1=9, P2=100)),                      # 3 P2 > 255: the wide three-path volume
]


@pytest.mark.parametrize("W,H,D,r,cmax,kw", E2E_CASES, ids=["%dx%d-D%d-r%d-%s" % (c[0], c[1], c[2], c[3], "+".join(sorted(c[5])) or "defaults") for c in E2E_CASES])
def test_census_handle_equals_the_definition_end_to_end(jn, oracle, W, H, D, r, cmax, kw):
    """jn_sgm_process_batch, and the same handle's producer fed to an EXTERNAL handle's consumer."""
    DeviceArray = _dev(jn)
    n = 2
    pairs = [oracle.synth_pair(W, H, min(D - 16, 40), 900 + b) for b in range(n)]
    Ls, Rs = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    p = jn.Sgm.parameters(num_disparities=D, **kw)
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    dD = DeviceArray((n, H, W), np.int16); dD2 = DeviceArray((n, H, W), np.int16); dD3 = DeviceArray((n, H, W), np.int16)
    dC = DeviceArray((n, H, W, D), np.uint8)
    with jn.Sgm(p, W, H, max_batch=n, cost=_census(jn, block_radius=r, cost_max=cmax)) as m, \
            jn.Sgm(p, W, H, max_batch=n, cost=jn.Sgm.cost_parameters(cost_function=cd.EXTERNAL)) as ext:
        m.process_batch(n, dL.ptr, dR.ptr, W, H * W, dD.ptr)
        t = m.last_times()
        m.cost_volume(n, dL.ptr, dR.ptr, W, H * W, dC.ptr)
        m.aggregate(n, dC.ptr, dD2.ptr)
        ext.aggregate(n, dC.ptr, dD3.ptr)
        assert m.debug_ptr(5)[0] is None                         # no prefiltered rows on a volume handle
    got = dD.numpy()
    assert np.array_equal(got, dD2.numpy()) and np.array_equal(got, dD3.numpy())
    for b in range(n):
        assert np.array_equal(got[b], cs.process(Ls[b], Rs[b], D, p.P1, p.P2, p.lr_max_diff, p.subpixel, r, cmax)), b
    assert (got >= 0).mean() > 0.3
    assert t["prefilter"] > 0 and t["total"] >= t["prefilter"]   # the producer is the `prefilter` stage
    for a in (dL, dR, dD, dD2, dD3, dC):
        a.free()


@pytest.mark.parametrize("sub,postfilter", [(0, False), (1, False), (1, True)])
def test_eight_pipelined_slots_with_the_scan_tail_equal_the_synchronous_route(jn, oracle, sub, postfilter):
    """jn_sgm_submit_scan on all eight slots at once (slots 1 .. 7 allocate their own volume and signatures): the int16 map, the mono8
    map, bins and meta must equal the synchronous call + jn_sgm_disparity_to_u8 + the stand-alone scan; once with the post-filter."""
    DeviceArray = _dev(jn)
    from jackal_navigation_amd import node, postfilter as pf
    W, H, D, n, S, r = 230, 60, 64, 2, 8, 4
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    frames = [[oracle.synth_pair(W, H, 40, 700 + 10 * k + t) for t in range(n)] for k in range(S)]
    dL = [DeviceArray.from_numpy(np.stack([f[0] for f in fs])) for fs in frames]
    dR = [DeviceArray.from_numpy(np.stack([f[1] for f in fs])) for fs in frames]
    p = jn.Sgm.parameters(num_disparities=D, subpixel=sub)
    fp = pf.postfilter_params(pf.I16_SUB if sub else pf.I16, speckle_size=40)
    with jn.Sgm(p, W, H, max_batch=n, cost=_census(jn, block_radius=r, cost_max=62)) as m:
        want = []
        for k in range(S):
            dd = DeviceArray((n, H, W), np.int16); du = DeviceArray((n, H, W), np.uint8)
            bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
            m.process_batch(n, dL[k].ptr, dR[k].ptr, W, H * W, dd.ptr)
            if postfilter:
                pf.disparity_postfilter(fp, n, dd.ptr, W, H)
            m.to_u8(dd.ptr, du.ptr, n * H * W)
            node.obstacle_scan(sp, n, du.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
            want.append(tuple(a.numpy().copy() for a in (dd, du, bins, meta)))
        outs = [tuple([DeviceArray((n, H, W), np.int16), DeviceArray((n, H, W), np.uint8), DeviceArray((n, sp.bins), np.float64),
                       DeviceArray((n, 4), np.float64)]) for _ in range(S)]
        for k in range(S):
            if postfilter:
                m.attach_postfilter(k, fp)
            o = outs[k]
            m.submit_scan(k, n, dL[k].ptr, dR[k].ptr, W, H * W, o[0].ptr, sp, lut.ptr, o[1].ptr, o[2].ptr, o[3].ptr)
        for k in range(S):
            m.wait(k)
        got = [tuple(a.numpy().copy() for a in outs[k]) for k in range(S)]
    for k in range(S):
        for a, b in zip(want[k], got[k]):
            assert np.array_equal(a, b), k
        assert (want[k][0] >= 0).mean() > 0.3
    if not postfilter:
        for k in (0, S - 1):
            assert np.array_equal(got[k][0][0], cs.process(frames[k][0][0], frames[k][0][1], D, p.P1, p.P2, p.lr_max_diff, sub, r, 62)), k


@pytest.mark.parametrize("table", ["gain", "gamma"])
@pytest.mark.parametrize("scene", ["blobs", "grain"])
def test_a_grey_scale_change_of_one_eye_leaves_the_census_map_untouched(jn, scene, table):
    """The reason the mode exists.  7-bit scenes; the right eye goes through a strictly increasing table (a gain with an offset, a
    gamma curve).  The census handle's map is the same bit for bit; the plain (Sobel + 1x3 SAD) handle's map of the same two pairs is not."""
    W, H, D = 240, 64, 64
    lut = cs.increasing_tables()[table]
    assert (np.diff(lut.astype(np.int64)) > 0).all()
    L, R = scenes.make_scene(scene, W, H, 40, 11)
    L, R = L >> 1, R >> 1
    R2 = lut[R]
    assert not np.array_equal(R2, R)
    p = jn.Sgm.parameters(num_disparities=D, subpixel=1)
    census = lambda pp, w, h, max_batch=1: jn.Sgm(pp, w, h, max_batch=max_batch, cost=_census(jn, block_radius=4, cost_max=62))
    a, _, _ = run(jn, census, p, np.stack([L, L]), np.stack([R, R2]))
    assert np.array_equal(a[0], a[1])
    assert np.array_equal(a[0], cs.process(L, R, D, p.P1, p.P2, p.lr_max_diff, 1, 4, 62))
    assert (a[0] >= 0).mean() > 0.3
    b, _, _ = run(jn, jn.Sgm, p, np.stack([L, L]), np.stack([R, R2]))
    assert not np.array_equal(b[0], b[1]), "the plain cost is not expected to survive the change: the test would prove nothing"


def test_the_other_costs_are_what_they_were_next_to_a_census_handle(jn, oracle):
    """A census handle, a BLOCK_SSD handle and a plain handle alive in one process: the latter two against their definitions."""
    DeviceArray = _dev(jn)
    from oracle.binding import SgmOracle
    W, H, D = 170, 48, 64
    L, R = oracle.synth_pair(W, H, 40, 77)
    p = jn.Sgm.parameters(num_disparities=D, subpixel=1)
    dL, dR = DeviceArray.from_numpy(L), DeviceArray.from_numpy(R)
    outs = [DeviceArray((1, H, W), np.int16) for _ in range(3)]
    with jn.Sgm(p, W, H, cost=_census(jn, block_radius=3)) as cen, jn.Sgm(p, W, H, cost=jn.Sgm.cost_parameters()) as blk, jn.Sgm(p, W, H) as plain:
        for _ in range(2):                                       # interleaved, twice
            for m, o in zip((cen, blk, plain), outs):
                m.process_batch(1, dL.ptr, dR.ptr, W, H * W, o.ptr)
    got = [o.numpy()[0] for o in outs]
    assert np.array_equal(got[0], cs.process(L, R, D, p.P1, p.P2, p.lr_max_diff, 1, 3, 127))
    assert np.array_equal(got[1], cd.process(L, R, D, p.P1, p.P2, p.prefilter_cap, p.lr_max_diff, 1, 2, 5, 127))
    assert np.array_equal(got[2], SgmOracle().process(SgmOracle.params(num_disparities=D, subpixel=1), L, R))
    for a in [dL, dR] + outs:
        a.free()

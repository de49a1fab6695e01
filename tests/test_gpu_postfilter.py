"""The disparity post-filter (include/jn_postfilter.h) on the GPU against its scalar definition (tests/postfilter_def.py): output and
statistics bit-identical everywhere — random maps, the shapes that break labelling schemes, real SGM and block-matching output, the
filter attached to SGM slots ahead of the scan, the costmap and the sub-pixel tail, the block-matching recipe, the phantom obstacle."""
import numpy as np
import pytest

import postfilter_def as pd
import subpix_def as sd

pytestmark = pytest.mark.gpu

FORMATS = (pd.I16, pd.I16_SUB)


def run(jn, fp, maps, in_place=True, stats=True):
    """maps [n][H][W] int16 through jn_disparity_postfilter -> (output, stats or None); out of place the input must come back untouched."""
    from jackal_navigation_amd import postfilter
    from jackal_navigation_amd.device import DeviceArray
    maps = np.ascontiguousarray(maps, np.int16)
    n, H, W = maps.shape
    d = DeviceArray.from_numpy(maps)
    o = d if in_place else DeviceArray.from_numpy(np.full(maps.shape, 12345, np.int16))
    s = DeviceArray.from_numpy(np.full((n, 4), 0xDEADBEEF, np.uint32)) if stats else None
    postfilter.disparity_postfilter(fp, n, d.ptr, W, H, None if in_place else o.ptr, s.ptr if stats else None)
    if not in_place:
        assert np.array_equal(d.numpy(), maps)
    return o.numpy(), (s.numpy() if stats else None)


def check(jn, maps, fmt, what, in_place=True, stats=True, **kw):
    from jackal_navigation_amd import postfilter
    want, wstats = pd.apply(maps, fmt, **{"speckle_size": 200, "speckle_range_q": 16, "median": 0, **kw})
    got, gstats = run(jn, postfilter.postfilter_params(fmt, **kw), maps, in_place, stats)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, kw, len(bad), bad[:5].tolist(), [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])
    if stats:
        assert np.array_equal(gstats, wstats), (what, kw, gstats.tolist(), wstats.tolist())
    return want, wstats


def planted(rng, n, H, W, fmt):
    """Noise with holes, rectangles of constant and of slowly varying disparity (segments of many sizes), isolated pixels."""
    unit = 1 if fmt == pd.I16 else 16
    m = rng.integers(0, 60, (n, H, W)) * unit + (rng.integers(0, 16, (n, H, W)) if fmt == pd.I16_SUB else 0)
    for f in range(n):
        for _ in range(24):
            x0, x1 = sorted(rng.integers(0, W, 2)); y0, y1 = sorted(rng.integers(0, H, 2))
            x1 = min(x1, x0 + 90); y1 = min(y1, y0 + 70)
            base = int(rng.integers(1, 100)) * unit
            ramp = (np.arange(x1 - x0 + 1)[None, :] // 3 + np.arange(y1 - y0 + 1)[:, None] // 2) * (unit if rng.random() < 0.5 else 0)
            m[f, y0:y1 + 1, x0:x1 + 1] = base + ramp
    m[rng.random((n, H, W)) < 0.12] = -unit
    m[rng.random((n, H, W)) < 0.01] = -7                           # an invalid value that is not the marker: copied through
    return np.clip(m, -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("W,H,n", [(320, 180, 3), (1280, 720, 2), (1919, 1079, 1), (8, 8, 1), (1, 300, 2), (300, 1, 2)])
def test_random_maps_equal_the_definition(jn, fmt, W, H, n):
    rng = np.random.default_rng(W * 7 + H + fmt)
    maps = planted(rng, n, H, W, fmt)
    small = W * H <= 320 * 180
    sizes = (0, 1, 2, 200, 1 << 24) if small else (200,)
    ranges = (0, 16, 4096) if small else (16,)
    k = 0
    for size in sizes:
        for rq in ranges:
            for median in (0, 1):
                k += 1
                _, st = check(jn, maps, fmt, ("random", W, H, n), in_place=k % 2 == 0, stats=k % 3 != 0, speckle_size=size, speckle_range_q=rq, median=median)
    _, st = check(jn, maps, fmt, ("random", W, H, n), speckle_size=50, speckle_range_q=16 if fmt == pd.I16 else 20, median=1, in_place=False)
    if min(W, H) > 8:                                               # some segments go, some stay
        assert st[:, 3].sum() > 0 and (st[:, 1] > st[:, 2]).all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_shapes_that_break_labelling_schemes(jn, fmt):
    W, H = 1280, 720
    unit = 1 if fmt == pd.I16 else 16
    one = np.full((1, H, W), 40 * unit, np.int16)
    _, st = check(jn, one, fmt, "one segment", speckle_size=1 << 20)         # 921 600 pixels: fewer than 2^20, removed whole
    assert st.tolist() == [[W * H, 1, 1, W * H]]
    _, st = check(jn, one, fmt, "one segment kept", speckle_size=W * H, median=1)
    assert st.tolist() == [[W * H, 1, 0, 0]]
    ramp = (np.arange(W)[None, :] + np.arange(H)[:, None]).astype(np.int16)[None] * (1 if fmt == pd.I16 else 16)
    _, st = check(jn, ramp, fmt, "ramp", speckle_size=W * H)                   # steps of one pixel: one segment of 0 .. 1998 px
    assert st[0, 1] == 1 and st[0, 3] == 0
    for name, m in (("spiral", pd.spiral(H, W)), ("serpentine", pd.serpentine(H, W))):
        m = np.where(m >= 0, m * unit, -unit).astype(np.int16)[None]
        for size in (200, 1 << 24):
            _, st = check(jn, m, fmt, name, speckle_size=size, median=int(size == 200))
            assert st[0, 1] == 1, (name, st.tolist())                          # the definition agrees that it is ONE chain
            assert st[0, 3] == (0 if size == 200 else st[0, 0])
    yy, xx = np.mgrid[0:H, 0:W]
    board = np.where((yy + xx) % 2 == 0, 30 * unit, -unit).astype(np.int16)[None]
    _, st = check(jn, board, fmt, "checkerboard", speckle_size=2)
    assert st.tolist() == [[W * H // 2] * 2 + [W * H // 2] * 2]
    check(jn, board, fmt, "checkerboard kept", speckle_size=1, median=1)
    check(jn, np.where(xx % 2 == 0, 30 * unit, -unit).astype(np.int16)[None], fmt, "vertical stripes", speckle_size=H + 1)
    check(jn, np.where(xx % 2 == 0, 30 * unit, -unit).astype(np.int16)[None], fmt, "vertical stripes kept", speckle_size=H)
    check(jn, np.where(yy % 2 == 0, 30 * unit, -unit).astype(np.int16)[None], fmt, "horizontal stripes", speckle_size=W + 1, median=1)
    check(jn, np.where(yy % 2 == 0, 30 * unit, -unit).astype(np.int16)[None], fmt, "horizontal stripes kept", speckle_size=W)
    # alternating values two pixels apart: no two neighbours connect at range 1, all connect at range 2
    alt = (((yy + xx) % 2) * 2 * unit + 10 * unit).astype(np.int16)[None]
    _, st = check(jn, alt, fmt, "alternating", speckle_size=2, speckle_range_q=16)
    assert st[0, 1] == W * H and st[0, 3] == W * H
    _, st = check(jn, alt, fmt, "alternating joined", speckle_size=2, speckle_range_q=32)
    assert st[0, 1] == 1 and st[0, 3] == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_frames_of_a_batch_do_not_leak_into_each_other(jn, fmt):
    W, H, n = 200, 37, 4
    unit = 1 if fmt == pd.I16 else 16
    m = np.full((n, H, W), -unit, np.int16)
    m[:, 0, 10:110] = 8 * unit                                      # 100 pixels in the first row and 100 in the last of EVERY frame:
    m[:, H - 1, 10:110] = 8 * unit                                  # 200 together if the last row of a frame met the first of the next
    _, st = check(jn, m, fmt, "leak", speckle_size=150)
    assert st.tolist() == [[200, 2, 2, 200]] * n
    _, st = check(jn, m, fmt, "no leak, kept", speckle_size=100, median=1)
    assert st.tolist() == [[200, 2, 0, 0]] * n
    _, st = check(jn, np.full((3, 50, 70), -unit, np.int16), fmt, "all invalid", median=1)
    assert st.tolist() == [[0, 0, 0, 0]] * 3


def _matcher_maps(jn, mode, kind, subpixel, W, H, B):
    """(handle class, parameters) -> the unfiltered maps [B][H][W] of scenes of one kind, through the synchronous batch call."""
    import scenes
    from jackal_navigation_amd.device import DeviceArray
    pairs = [scenes.make_scene(kind, W, H, 48, 500 + t) for t in range(B)]
    dL = DeviceArray.from_numpy(np.stack([p[0] for p in pairs])); dR = DeviceArray.from_numpy(np.stack([p[1] for p in pairs]))
    dd = DeviceArray((B, H, W), np.int16)
    if mode == "sgm":
        h = jn.Sgm(jn.Sgm.parameters(num_disparities=64, subpixel=subpixel), W, H, max_batch=B)
    else:
        h = jn.Bm(jn.Bm.parameters(num_disparities=64, subpixel=subpixel, cost_function=1 if mode == "bm_ssd" else 0), W, H, max_batch=B)
    with h:
        h.process_batch(B, dL.ptr, dR.ptr, W, H * W, dd.ptr)
    return dd.numpy()


@pytest.mark.parametrize("subpixel", [0, 1])
@pytest.mark.parametrize("mode", ["sgm", "bm_sad", "bm_ssd"])
def test_real_matcher_output(jn, mode, subpixel):
    fmt = pd.I16_SUB if subpixel else pd.I16
    removed = 0
    for kind in ("strips", "blobs", "periodic"):
        maps = _matcher_maps(jn, mode, kind, subpixel, 320, 180, 2)
        assert (maps >= 0).any()
        _, st = check(jn, maps, fmt, (mode, kind, subpixel), speckle_size=200, speckle_range_q=16)
        removed += int(st[:, 3].sum())
        check(jn, maps, fmt, (mode, kind, subpixel, "median"), speckle_size=60, speckle_range_q=24, median=1, in_place=False)
    assert removed > 0                                              # otherwise this test shows nothing


@pytest.mark.parametrize("subpixel", [0, 1])
def test_attached_to_sgm_slots(jn, subpixel):
    """Two slots in flight with the filter ahead of the mono8 map, the scan, an attached costmap and an attached sub-pixel tail: dDisp is the
    definition of the unfiltered map, every consumer's output is what the synchronous entry points make of the filtered dDisp, and after
    detaching the slot is bit-identical to one that never had a filter."""
    from jackal_navigation_amd import costmap, node, postfilter, subpix
    from jackal_navigation_amd.device import DeviceArray
    import scenes
    W, H, B, S = 320, 180, 2, 2
    fmt = pd.I16_SUB if subpixel else pd.I16
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    cp = costmap.costmap_params(min_hits=2)
    pairs = [[scenes.make_scene(("blobs", "strips")[s], W, H, 48, 70 + 10 * s + t) for t in range(B)] for s in range(S)]
    dL = [DeviceArray.from_numpy(np.stack([p[0] for p in ps])) for ps in pairs]
    dR = [DeviceArray.from_numpy(np.stack([p[1] for p in ps])) for ps in pairs]
    names = ("dd", "u8", "bins", "meta", "hits", "grid", "xbins", "xmeta", "xhits", "xgrid")

    def buffers():
        return dict(dd=DeviceArray((B, H, W), np.int16), u8=DeviceArray((B, H, W), np.uint8), bins=DeviceArray((B, sp.bins), np.float64),
                    meta=DeviceArray((B, 4), np.float64), hits=DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16),
                    grid=DeviceArray((B, cp.cells_y, cp.cells_x), np.int8), xbins=DeviceArray((B, sp.bins), np.float64),
                    xmeta=DeviceArray((B, 4), np.float64), xhits=DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16),
                    xgrid=DeviceArray((B, cp.cells_y, cp.cells_x), np.int8), stats=DeviceArray((B, 4), np.uint32))
    bufs = [buffers() for _ in range(S)]

    def submit_all(m, scan=True):
        for s in range(S):
            b = bufs[s]
            for k in names:
                b[k].upload(np.full(b[k].shape, 77, b[k].dtype))
            if scan:
                m.submit_scan(s, B, dL[s].ptr, dR[s].ptr, W, H * W, b["dd"].ptr, sp, lut.ptr, b["u8"].ptr, b["bins"].ptr, b["meta"].ptr)
            else:
                m.submit_scan(s, B, dL[s].ptr, dR[s].ptr, W, H * W, b["dd"].ptr)
        for s in range(S):
            m.wait(s)
        return [{k: bufs[s][k].numpy().copy() for k in names + ("stats",)} for s in range(S)]

    def same(a, b):
        return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))

    kw = [dict(speckle_size=200, speckle_range_q=16, median=0), dict(speckle_size=80, speckle_range_q=32, median=1)]
    with jn.Sgm(jn.Sgm.parameters(num_disparities=64, subpixel=subpixel), W, H, max_batch=B) as m:
        for s in range(S):
            costmap.attach(m, s, cp, bufs[s]["hits"].ptr, bufs[s]["grid"].ptr)
            m.attach_subpix(s, cp, bufs[s]["xbins"].ptr, bufs[s]["xmeta"].ptr, bufs[s]["xhits"].ptr, bufs[s]["xgrid"].ptr)
        plain = submit_all(m)
        plain_noscan = submit_all(m, scan=False)
        for s in range(S):
            assert same(plain[s]["dd"], plain_noscan[s]["dd"])
        m.attach_postfilter(0, postfilter.postfilter_params(fmt, **kw[0]), bufs[0]["stats"].ptr)
        postfilter.attach(m, 1, postfilter.postfilter_params(fmt, **kw[1]), bufs[1]["stats"].ptr)
        other = pd.I16 if subpixel else pd.I16_SUB
        for bad in ((8, postfilter.postfilter_params(fmt)), (-1, postfilter.postfilter_params(fmt)), (0, postfilter.postfilter_params(other)),
                    (0, postfilter.postfilter_params(fmt, median=2)), (0, postfilter.postfilter_params(fmt, speckle_size=-1))):
            with pytest.raises(jn.JnError):
                m.attach_postfilter(*bad)
        removed = 0
        for rep in range(2):
            for scan in (True, False):
                got = submit_all(m, scan)
                for s in range(S):
                    want, wstats = pd.apply(plain[s]["dd"], fmt, **kw[s])
                    assert np.array_equal(got[s]["dd"], want), (s, rep, scan)
                    assert np.array_equal(got[s]["stats"], wstats), (s, rep, scan)
                    removed += int(wstats[:, 3].sum())
                    if not scan:                                           # nothing but the map is written without scan parameters
                        assert all((got[s][k] == 77).all() for k in names[1:])
                        continue
                    # what the synchronous entry points make of the filtered map
                    dd = DeviceArray.from_numpy(want); u8 = DeviceArray((B, H, W), np.uint8)
                    bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
                    hits = DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)
                    m.to_u8(dd.ptr, u8.ptr, B * W * H)
                    node.obstacle_scan(sp, B, u8.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
                    costmap.obstacle_costmap(sp, cp, B, u8.ptr, lut.ptr, W, H, bins.ptr, hits.ptr, grid.ptr)
                    for k, ref in (("u8", u8), ("bins", bins), ("meta", meta), ("hits", hits), ("grid", grid)):
                        assert same(got[s][k], ref.numpy()), (k, s, rep)
                    subpix.subpix_costmap(sp, cp, subpix.subpix_params(fmt), B, dd.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr)
                    for k, ref in (("xbins", bins), ("xmeta", meta), ("xhits", hits), ("xgrid", grid)):
                        assert same(got[s][k], ref.numpy()), (k, s, rep)
        assert removed > 0
        # a batch in flight refuses the call
        b = bufs[0]
        m.submit_scan(0, B, dL[0].ptr, dR[0].ptr, W, H * W, b["dd"].ptr)
        with pytest.raises(jn.JnError):
            m.attach_postfilter(0)
        m.wait(0)
        m.attach_postfilter(0)                                              # detach slot 0: it queues what it queued before
        got = submit_all(m)
        for k in names:
            assert same(got[0][k], plain[0][k]), k
        assert not same(got[1]["dd"], plain[1]["dd"])
        m.attach_postfilter(1, None)
        got = submit_all(m)
        for s in range(S):
            for k in names:
                assert same(got[s][k], plain[s][k]), (s, k)


@pytest.mark.parametrize("subpixel", [0, 1])
def test_the_block_matching_recipe(jn, subpixel):
    """jn_bm_submit_scan(sp = NULL), jn_bm_wait, jn_disparity_postfilter in place, then the mono8 map and the scan, or the sub-pixel grid."""
    from jackal_navigation_amd import costmap, node, postfilter, subpix
    from jackal_navigation_amd.device import DeviceArray
    import scenes
    W, H, B = 320, 180, 2
    fmt = pd.I16_SUB if subpixel else pd.I16
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    cp = costmap.costmap_params()
    pairs = [scenes.make_scene("blobs", W, H, 48, 900 + t) for t in range(B)]
    dL = DeviceArray.from_numpy(np.stack([p[0] for p in pairs])); dR = DeviceArray.from_numpy(np.stack([p[1] for p in pairs]))
    dd = DeviceArray((B, H, W), np.int16); u8 = DeviceArray((B, H, W), np.uint8); st = DeviceArray((B, 4), np.uint32)
    bins = DeviceArray((B, sp.bins), np.float64); meta = DeviceArray((B, 4), np.float64)
    hits = DeviceArray((B, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((B, cp.cells_y, cp.cells_x), np.int8)
    fp = postfilter.postfilter_params(fmt, speckle_size=150)
    with jn.Bm(jn.Bm.parameters(num_disparities=64, subpixel=subpixel), W, H, max_batch=B) as m:
        with pytest.raises(TypeError, match="disparity_postfilter"):
            postfilter.attach(m, 1, fp)
        m.submit_scan(1, B, dL.ptr, dR.ptr, W, H * W, dd.ptr)
        m.wait(1)
        raw = dd.numpy()
        postfilter.disparity_postfilter(fp, B, dd.ptr, W, H, None, st.ptr)
        m.to_u8(dd.ptr, u8.ptr, B * W * H)
        node.obstacle_scan(sp, B, u8.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
    want, wstats = pd.apply(raw, fmt, speckle_size=150)
    assert np.array_equal(dd.numpy(), want) and np.array_equal(st.numpy(), wstats) and wstats[:, 3].sum() > 0
    # the mono8 map of the filtered map: invalid -> 0, 1/16 pixel rounded half to even, saturating
    w = want.astype(np.int64)
    ref = np.where(w < 0, 0, np.minimum(np.rint(w / 16.0) if subpixel else w, 255)).astype(np.uint8)
    assert np.array_equal(u8.numpy(), ref)
    assert (bins.numpy() < sd.EMPTY - 1).any()
    subpix.subpix_costmap(sp, cp, subpix.subpix_params(fmt), B, dd.ptr, W, H, bins.ptr, meta.ptr, hits.ptr, grid.ptr)
    q, v = sd.to_q(want, fmt)
    for f in range(B):
        assert np.array_equal(hits.numpy()[f], sd.hits(sp, cp, q[f], v[f]))


def test_the_phantom_obstacle_on_the_device(jn):
    """A wall at 3 m with a 12-pixel blob at 0.8 m: the sub-pixel scan's bin reads 0.8 m before the filter and the wall's range after."""
    from jackal_navigation_amd import node, postfilter, subpix
    from jackal_navigation_amd.device import DeviceArray
    W, H = 320, 180
    sp = node.scan_params(W, H)
    wall, _ = sd.wall_q(sp, W, H, 3.0)
    near, _ = sd.wall_q(sp, W, H, 0.8)
    m = wall.astype(np.int16)
    m[60:63, 158:162] = near[0, 0]
    m = m[None]
    bins_w, _, _ = sd.scan(sp, wall, np.ones((H, W), bool))
    dd = DeviceArray.from_numpy(m); bins = DeviceArray((1, sp.bins), np.float64); meta = DeviceArray((1, 4), np.float64)
    fpx = subpix.subpix_params(subpix.I16_SUB)
    subpix.subpix_scan(sp, fpx, 1, dd.ptr, W, H, bins.ptr, meta.ptr)
    before = bins.numpy()[0]
    k = int(np.argmin(before))
    assert 0.7 < before[k] < 0.9 and bins_w[k] > 2.5
    st = DeviceArray((1, 4), np.uint32)
    postfilter.disparity_postfilter(postfilter.postfilter_params(pd.I16_SUB), 1, dd.ptr, W, H, None, st.ptr)
    assert st.numpy().tolist() == [[W * H, 2, 1, 12]]
    subpix.subpix_scan(sp, fpx, 1, dd.ptr, W, H, bins.ptr, meta.ptr)
    after = bins.numpy()[0]
    assert after.min() > 2.5 and abs(after[k] - bins_w[k]) < 0.05

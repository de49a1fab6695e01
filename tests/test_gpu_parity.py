"""Parity of the HIP path with the CPU oracle, through the C-ABI (libjn_stereo.so), on a real MI355X.

Bar: D1/D2 float disparities bit-identical (they are exact IEEE replays of the reference's
arithmetic), u8 maps identical, scan ranges within 1e-4 (north star: "float reprojection within
1e-4"; in practice they come out bit-identical or 1 ulp apart because atan2/sqrt are the device's)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCAN_TOL = 1e-4


def run_elas(jn, p, L, R, fill=0.0, **kw):
    H, W = L.shape
    D1 = np.full((H, W), fill, np.float32)
    D2 = np.full((H, W), fill, np.float32)
    with jn.Elas(p, W, H, **kw) as e:
        st = e.process(np.ascontiguousarray(L), np.ascontiguousarray(R), D1, D2, (W, H, W))
    return st, D1, D2


@pytest.mark.parametrize("name", ["elas_160x120_d63_seed7", "elas_320x180_d255_seed12345"])
def test_against_reference_golden_vectors(jn, golden, same, name):
    g = golden(name)
    st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=int(g["disp_max"])), g["L"], g["R"])
    assert st == 0 and same(D1, g["D1"]) and same(D2, g["D2"])


@pytest.mark.parametrize("W,H,sd,dmax,seed", [
    (320, 180, 48, 255, 12345),      # the reference node's native size and disparity range
    (640, 480, 64, 63, 12345),       # BASELINE config 2
    (1280, 720, 128, 127, 12345),    # BASELINE config 3 frame size
    (333, 201, 30, 95, 5),           # ragged: width not a multiple of 16, odd height
    (256, 64, 20, 40, 2),            # very flat image
    (100, 100, 12, 30, 8),           # tiny
])
def test_elas_bit_exact_vs_oracle(jn, oracle, same, W, H, sd, dmax, seed):
    L, R = jn.node.synth_pair(W, H, sd, seed)
    st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=dmax), L, R)
    st_o, D1o, D2o = oracle.process(oracle.params(0, disp_max=dmax), L, R)
    assert st == st_o
    assert same(D1, D1o), "%d differing pixels in D1" % int((D1 != D1o).sum())
    assert same(D2, D2o), "%d differing pixels in D2" % int((D2 != D2o).sum())


@pytest.mark.parametrize("kind", ["strips", "patches", "slanted", "photometric", "blobs", "shallow", "grain", "periodic"])
def test_other_scenes_bit_exact_vs_oracle(jn, oracle, same, kind):
    """Scenes unlike the survey's plane-and-box generator (tests/scenes.py; the oracle is pinned against the reference
    on them in test_oracle_vs_reference.py): occlusions and depth jumps, textureless patches, slanted surfaces,
    photometric differences, random blobs — as a batch through the pipelined API, one of them at 1280x720."""
    from scenes import make_scene
    from jackal_navigation_amd.device import DeviceArray
    for (W, H, dmax, n) in ((320, 240, 79, 5), (640, 360, 95, 3), (1280, 720, 127, 2)):
        pairs = [make_scene(kind, W, H, dmax, 50 + b) for b in range(n)]
        Ls = np.stack([p[0] for p in pairs]); Rs = np.stack([p[1] for p in pairs])
        dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
        d1 = DeviceArray((n, H, W), np.float32); d2 = DeviceArray((n, H, W), np.float32)
        with jn.Elas(jn.Elas.parameters(0, disp_max=dmax, postprocess_only_left=0), W, H, max_batch=n, host_threads=2) as e:
            assert e.process_batch(n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr) == [0] * n
        D1, D2 = d1.numpy(), d2.numpy()
        po = oracle.params(0, disp_max=dmax, postprocess_only_left=0)
        for b in range(n):
            _, D1o, D2o = oracle.process(po, Ls[b], Rs[b])
            assert same(D1[b], D1o) and same(D2[b], D2o), (kind, W, H, b, int((D1[b] != D1o).sum()), int((D2[b] != D2o).sum()))
        for a in (dL, dR, d1, d2):
            a.free()


def test_full_hd_and_wide_images(jn, oracle, same):
    """BASELINE config 5's frame (1920x1080, disparity range 256: the widest LDS windows) and an image wider than
    2560 px: since lattice rows are cut into segments it stays in the LDS kernel and the plane flow (eight segments of 65 candidates, windows of
    459 columns in the 640 bucket); the global-memory kernel k_support runs in tests/test_gpu_elas_matrix.py (JN_SUPPORT_SEGMENTS=1, hooks build)."""
    for (W, H, sd, dmax, seed) in ((1920, 1080, 256, 255, 12345), (2600, 200, 40, 63, 3)):
        L, R = jn.node.synth_pair(W, H, sd, seed)
        st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=dmax), L, R)
        st_o, D1o, D2o = oracle.process(oracle.params(0, disp_max=dmax), L, R)
        assert st == st_o == 0 and same(D1, D1o) and same(D2, D2o), (W, H)
    import os
    # SURVEY.md §8c known answer for 1920x1080, scene d<=256, disp_max=255 (measured there on the reference itself)
    L, R = jn.node.synth_pair(1920, 1080, 256, 12345)
    _, D1, _ = run_elas(jn, jn.Elas.parameters(0, disp_max=255), L, R)
    assert oracle.fnv(D1) == 0xcd2740a7ac6afdf7


def test_known_answer_hashes_on_gpu(jn, oracle):
    import os
    rows = [l.split() for l in open(os.path.join(os.path.dirname(__file__), "golden", "reference_hashes.txt")) if not l.startswith("#")]
    for W, H, sd, dmax, h1, h2 in rows:
        L, R = jn.node.synth_pair(int(W), int(H), int(sd), 12345)
        st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=int(dmax)), L, R)
        assert st == 0 and oracle.fnv(D1) == int(h1, 16) and oracle.fnv(D2) == int(h2, 16), (W, H)


def test_known_answer_hashes_on_other_scenes_on_gpu(jn, oracle):
    """HIP path against the REFERENCE's own hashes (tests/golden/reference_scene_hashes.txt) on the scene kinds of
    tests/scenes.py, both sides post-processed."""
    import os
    from scenes import make_scene
    rows = [l.split() for l in open(os.path.join(os.path.dirname(__file__), "golden", "reference_scene_hashes.txt")) if not l.startswith("#")]
    assert len(rows) >= 12
    for kind, W, H, dmax, seed, h1, h2 in rows:
        L, R = make_scene(kind, int(W), int(H), int(dmax), int(seed))
        st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=int(dmax), postprocess_only_left=0), L, R)
        assert st == 0 and oracle.fnv(D1) == int(h1, 16) and oracle.fnv(D2) == int(h2, 16), (kind, W, H)


@pytest.mark.parametrize("kw", [
    {"postprocess_only_left": 0}, {"filter_adaptive_mean": 0}, {"ipol_gap_width": 7}, {"speckle_size": 50, "speckle_sim_threshold": 2.0},
    {"support_threshold": 0.95, "support_texture": 20}, {"lr_threshold": 1, "match_texture": 5}, {"grid_size": 16, "sradius": 3.0},
    {"candidate_stepsize": 4, "incon_window_size": 3, "incon_min_support": 3}, {"gamma": 5.0, "beta": 0.03, "sigma": 1.5},
    {"filter_median": 1}, {"filter_median": 1, "filter_adaptive_mean": 0, "postprocess_only_left": 0},
    {"disp_min": 6}, {"disp_min": 20, "postprocess_only_left": 0}, {"disp_min": -5}, {"disp_min": 70},   # the last: no candidate has 10 disparities left -> no support points
])
def test_parameter_variations(jn, oracle, same, kw):
    W, H = 320, 240
    L, R = jn.node.synth_pair(W, H, 40, 21)
    st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=79, **kw), L, R)
    st_o, D1o, D2o = oracle.process(oracle.params(0, disp_max=79, **kw), L, R)
    assert st == st_o and same(D1, D1o) and same(D2, D2o), kw
    assert st == (1 if kw.get("disp_min", 0) == 70 else 0)                      # JN_ERR_FEW_SUPPORT: outputs untouched, as elas.cpp:66-71


def test_support_filters_on_device_and_on_host_agree(jn, hooks, oracle, same, monkeypatch):
    """The support-point filters run in k_support_filters when the lattice fits its LDS wavefront and on the host
    workers otherwise; by default lone pairs also go to the host, which is faster for latency (JN_HOST_FILTERS=0/1 forces a route
    at create time).  Both routes must give the oracle's maps,
    also with a non-default tolerance / support count and with a window size the kernel does not take."""
    W, H = 640, 360
    L, R = jn.node.synth_pair(W, H, 64, 77)
    for kw in ({}, {"incon_threshold": 3, "incon_min_support": 9}, {"incon_window_size": 4}):
        _, D1o, D2o = oracle.process(oracle.params(0, disp_max=95, **kw), L, R)
        for host in (False, True):
            monkeypatch.setenv("JN_HOST_FILTERS", "1" if host else "0")      # unset = by batch size
            st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=95, **kw), L, R)
            assert st == 0 and same(D1, D1o) and same(D2, D2o), (kw, host)
    # the device route has two forms: classification + in-order resolution of the undecided points (default when
    # lattice and codes fit the LDS) and the skewed wavefront (JN_FILTER_WAVEFRONT=1, read once per process, so the
    # wavefront is exercised through the LDS budget below, which the default form does not fit)
    # lattices larger than the LDS are streamed through it in column / row pieces (1920x1080 does that for real);
    # a small LDS budget forces the same code on this small image, with 2 and with 5 column pieces
    monkeypatch.setenv("JN_HOST_FILTERS", "0")
    _, D1o, D2o = oracle.process(oracle.params(0, disp_max=95), L, R)
    for kb in ("16", "12", "6"):          # 16: codes + lattice do not fit, codes alone do (resolution from memory); 6: wavefront in pieces
        monkeypatch.setenv("JN_FILTER_LDS_KB", kb)
        st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=95), L, R)
        assert st == 0 and same(D1, D1o) and same(D2, D2o), kb


@pytest.mark.parametrize("form", [1, 2])
def test_device_filters_on_random_lattices(jn, oracle, same, form):
    """The filter kernels alone (jn_device_support_filters) on random lattices, where — unlike in stereo scenes —
    a large share of the points is undecided after classification and deletions cascade along the sweep: sparse, medium
    and dense lattices, several tolerances and support counts, a batch of different lattices at once."""
    from jackal_navigation_amd import _lib
    rng = np.random.default_rng(17 + form)
    L = jn.load()
    for (cw, ch, tol, sup, dmax) in ((80, 60, 5, 5, 60), (128, 96, 5, 5, 20), (67, 41, 3, 9, 40), (256, 144, 5, 5, 128), (50, 50, 1, 3, 8)):
        n = 6
        D = rng.integers(0, dmax, (n, ch, cw)).astype(np.int16)
        for b in range(n):
            D[b][rng.random((ch, cw)) < (0.05, 0.3, 0.5, 0.7, 0.85, 0.95)[b]] = -1     # from dense to almost empty
        D[:, 0, :] = 0; D[:, :, 0] = 0                                                   # elas.cpp:388-397
        p = jn.Elas.parameters(0, incon_threshold=tol, incon_min_support=sup)
        po = oracle.params(0, incon_threshold=tol, incon_min_support=sup)
        out = np.ascontiguousarray(D.copy())
        st = L.jn_device_support_filters(0, C.byref(p), cw * 5, ch * 5, n, out.ctypes.data, form)
        assert st == _lib.JN_OK, (cw, ch, form, st)
        for b in range(n):
            exp = oracle.remove_inconsistent(po, D[b])
            exp = oracle.remove_redundant(exp, 5, 1, True)
            exp = oracle.remove_redundant(exp, 5, 1, False)
            assert same(out[b], exp), (cw, ch, tol, sup, b, int((out[b] != exp).sum()))


def test_pitch_larger_than_width(jn, oracle, same):
    W, H, pitch = 300, 160, 352
    L, R = jn.node.synth_pair(W, H, 30, 4)
    Lp = np.zeros((H, pitch), np.uint8); Rp = np.zeros((H, pitch), np.uint8)
    Lp[:, :W] = L; Rp[:, :W] = R; Lp[:, W:] = 200; Rp[:, W:] = 17         # garbage in the padding must not matter
    D1 = np.zeros((H, W), np.float32); D2 = np.zeros((H, W), np.float32)
    with jn.Elas(jn.Elas.parameters(0, disp_max=63), W, H) as e:
        assert e.process(Lp, Rp, D1, D2, (W, H, pitch)) == 0
    _, D1o, D2o = oracle.process(oracle.params(0, disp_max=63), L, R)
    assert same(D1, D1o) and same(D2, D2o)


def test_too_few_support_points_leaves_outputs_untouched(jn):
    rng = np.random.default_rng(3)
    L = rng.integers(0, 255, (120, 160)).astype(np.uint8)
    R = rng.integers(0, 255, (120, 160)).astype(np.uint8)
    st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=63), L, R, fill=7.0)
    assert st == 1 and (D1 == 7).all() and (D2 == 7).all()             # elas.cpp:66-71
    flat = np.full((120, 160), 90, np.uint8)                           # no texture at all
    st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, disp_max=63), flat, flat, fill=-3.0)
    assert st == 1 and (D1 == -3).all()


def test_batch_device_pointers_with_a_failing_frame(jn, oracle, same):
    from jackal_navigation_amd.device import DeviceArray
    W, H, n = 320, 180, 5
    rng = np.random.default_rng(1)
    Ls = np.zeros((n, H, W), np.uint8); Rs = np.zeros((n, H, W), np.uint8)
    for b in range(n):
        Ls[b], Rs[b] = jn.node.synth_pair(W, H, 48, 500 + b)
    Ls[2] = rng.integers(0, 255, (H, W)); Rs[2] = rng.integers(0, 255, (H, W))    # frame 2: noise -> few support points
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    dD1 = DeviceArray.from_numpy(np.full((n, H, W), 5.0, np.float32)); dD2 = DeviceArray.from_numpy(np.full((n, H, W), 5.0, np.float32))
    p = jn.Elas.parameters(0)
    with jn.Elas(p, W, H, max_batch=n, host_threads=4, slots=2) as e:
        status = e.process_batch(n, dL.ptr, dR.ptr, W, H * W, dD1.ptr, dD2.ptr)
        D1, D2 = dD1.numpy(), dD2.numpy()
        # pipelined form gives the same answer
        dE1 = DeviceArray.from_numpy(np.full((n, H, W), 5.0, np.float32)); dE2 = DeviceArray.from_numpy(np.full((n, H, W), 5.0, np.float32))
        st_arr = (C.c_int32 * n)()
        e.submit(1, n, dL.ptr, dR.ptr, W, H * W, dE1.ptr, dE2.ptr, st_arr)
        e.wait(1)
        assert list(st_arr) == status and same(dE1.numpy(), D1) and same(dE2.numpy(), D2)
        times = e.last_times(1)
        assert times["total"] > 0 and times["host_stage"] >= 0       # (0: a batch handle triangulates on the GPU, there is no host stage)
    assert status == [0, 0, 1, 0, 0]
    assert (D1[2] == 5).all() and (D2[2] == 5).all()
    po = oracle.params(0)
    for b in (0, 1, 3, 4):
        _, D1o, D2o = oracle.process(po, Ls[b], Rs[b])
        assert same(D1[b], D1o) and same(D2[b], D2o), b


def test_slots_in_flight_do_not_interfere(jn, oracle, same):
    """Three batches of different pairs in flight on three slots (their kernels and host stages overlap, as in
    bench.py), for several rounds: every output equals what the same batch gives when it runs alone."""
    from jackal_navigation_amd.device import DeviceArray
    W, H, n, S = 320, 240, 6, 3
    p = jn.Elas.parameters(0, disp_max=79)
    batches = []
    for s in range(S):
        Ls = np.stack([jn.node.synth_pair(W, H, 30 + 10 * s, 7000 + 10 * s + b)[0] for b in range(n)])
        Rs = np.stack([jn.node.synth_pair(W, H, 30 + 10 * s, 7000 + 10 * s + b)[1] for b in range(n)])
        batches.append((Ls, Rs, DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)))
    with jn.Elas(p, W, H, max_batch=n, host_threads=4, slots=S) as e:      # 6 pairs > 4 pool threads: device filters
        alone = []
        for Ls, Rs, dL, dR in batches:
            d1 = DeviceArray((n, H, W), np.float32); d2 = DeviceArray((n, H, W), np.float32)
            assert e.process_batch(n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr) == [0] * n
            alone.append((d1.numpy(), d2.numpy()))
        outs = [(DeviceArray((n, H, W), np.float32), DeviceArray((n, H, W), np.float32)) for _ in range(S)]
        for rounds in range(4):
            for s in range(S):
                e.submit(s, n, batches[s][2].ptr, batches[s][3].ptr, W, H * W, outs[s][0].ptr, outs[s][1].ptr)
            for s in range(S):
                e.wait(s)
                assert same(outs[s][0].numpy(), alone[s][0]) and same(outs[s][1].numpy(), alone[s][1]), (rounds, s)
    _, D1o, D2o = oracle.process(oracle.params(0, disp_max=79), batches[1][0][3], batches[1][1][3])
    assert same(alone[1][0][3], D1o) and same(alone[1][1][3], D2o)


def test_full_size_batch_properties(jn, oracle, same):
    """BASELINE config 3 at full size (1280x720, D=128, batch 32): three frames bit-checked against the
    oracle (frame 4 has pixels claimed by two triangles: the reference's visiting order decides), every frame checked through size-independent properties — determinism (two runs agree),
    invalid value is exactly -10, and >= 99% of valid pixels within 1 of the synthetic ground truth."""
    from jackal_navigation_amd.device import DeviceArray
    W, H, n, D = 1280, 720, 32, 128
    Ls = np.zeros((n, H, W), np.uint8); Rs = np.zeros((n, H, W), np.uint8)
    for b in range(n):
        Ls[b], Rs[b] = jn.node.synth_pair(W, H, D, 12345 + b)
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    outs = []
    with jn.Elas(jn.Elas.parameters(0, disp_max=D - 1), W, H, max_batch=n, slots=2) as e:
        for rep in range(2):
            dD1 = DeviceArray.from_numpy(np.zeros((n, H, W), np.float32)); dD2 = DeviceArray.from_numpy(np.zeros((n, H, W), np.float32))
            assert e.process_batch(n, dL.ptr, dR.ptr, W, H * W, dD1.ptr, dD2.ptr) == [0] * n
            outs.append((dD1.numpy(), dD2.numpy()))
            dD1.free(); dD2.free()
    assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])
    D1 = outs[0][0]
    yy, xx = np.mgrid[0:H, 0:W]
    gt = (yy / H * (D * 0.6)).astype(int) + 2
    gt[(xx > W // 3) & (xx < W // 2) & (yy > H // 3) & (yy < 2 * H // 3)] = int(D * 0.7)
    for b in range(n):
        valid = D1[b] >= 0
        assert set(np.unique(D1[b][~valid]).tolist()) <= {-10.0}
        assert valid.mean() > 0.75
        assert (np.abs(D1[b][valid] - gt[valid]) <= 1.0).mean() > 0.99
    po = oracle.params(0, disp_max=D - 1)
    for b in (0, 4, 17):
        _, D1o, D2o = oracle.process(po, Ls[b], Rs[b])
        assert same(D1[b], D1o) and same(outs[0][1][b], D2o), b


def test_node_functions_vs_oracle(jn, oracle, same):
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node
    W, H, n = 320, 180, 3
    sp, spo = node.scan_params(W, H), oracle.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    luto = oracle.valid_lut(spo, W, H)
    assert same(lut.numpy(), luto)
    Ds = []
    for b in range(n):
        L, R = node.synth_pair(W, H, 48, 40 + b)
        _, D1, _ = oracle.process(oracle.params(0), L, R)
        Ds.append(D1)
    Ds = np.stack(Ds)
    Ds[2, 10, 10] = 254.5; Ds[2, 10, 11] = 300.0; Ds[2, 10, 12] = 2.5; Ds[2, 10, 13] = 3.5      # rounding / saturation probes
    dD = DeviceArray.from_numpy(Ds)
    du8 = DeviceArray((n, H, W), np.uint8); bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    node.disparity_scan(sp, n, dD.ptr, lut.ptr, W, H, du8.ptr, bins.ptr, meta.ptr)
    u8 = du8.numpy()
    b_, m_ = bins.numpy(), meta.numpy()
    for b in range(n):
        u8o = oracle.to_u8(Ds[b])
        assert same(u8[b], u8o)
        bo, mo, used = oracle.scan(spo, u8o, luto)
        assert used > 0
        assert np.array_equal(b_[b] < 1e9 - 1, bo < 1e9 - 1)
        assert np.allclose(b_[b], bo, rtol=0, atol=SCAN_TOL) and np.allclose(m_[b], mo, rtol=0, atol=SCAN_TOL)
        assert np.array_equal(node.compact_ranges(b_[b]) != 0, oracle.compact(bo) != 0)
    # separate entry points: u8 conversion alone, scan from a u8 map, point cloud
    du8b = DeviceArray((n, H, W), np.uint8)
    node.disparity_to_u8(dD.ptr, du8b.ptr, n * H * W)
    assert same(du8b.numpy(), u8)
    bins2 = DeviceArray((n, sp.bins), np.float64); meta2 = DeviceArray((n, 4), np.float64)
    node.obstacle_scan(sp, n, du8.ptr, lut.ptr, W, H, bins2.ptr, meta2.ptr)
    assert same(bins2.numpy(), b_) and same(meta2.numpy(), m_)
    bins3 = DeviceArray((n, sp.bins), np.float64); meta3 = DeviceArray((n, 4), np.float64)
    node.obstacle_scan_cloud(sp, n, du8.ptr, W, H, bins3.ptr, meta3.ptr)          # -g flavour: d >= 2, ground model instead of the LUT
    for b in range(n):
        bo, mo, used = oracle.scan_cloud(spo, u8[b])
        assert used > 0 and np.array_equal(bins3.numpy()[b] < 1e9 - 1, bo < 1e9 - 1)
        assert np.allclose(bins3.numpy()[b], bo, rtol=0, atol=SCAN_TOL) and np.allclose(meta3.numpy()[b], mo, rtol=0, atol=SCAN_TOL)
    pc = node.point_cloud(sp, du8.ptr, W, H)            # first map
    pco = oracle.point_cloud(spo, u8[0])
    assert pc.shape == pco.shape and np.allclose(pc, pco, rtol=0, atol=SCAN_TOL)
    msg = node.laser_scan_message(b_[0], m_[0], seq=3)
    assert msg["header"]["frame_id"] == "jackal" and len(msg["ranges"]) == int((b_[0] < 1e9 - 1).sum())


def test_scans_drive_the_same_navigation_decisions(jn, oracle):
    """raw pairs -> HIP ELAS -> u8 -> scan -> LaserScan -> navigate.cpp's consumer, beside the same
    chain on the oracle.  Scans agree to 1e-4 (device atan2/sqrt), the decisions taken from them must be equal."""
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node, navigate
    W, H, n = 320, 180, 12
    sp, spo = node.scan_params(W, H), oracle.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    luto = oracle.valid_lut(spo, W, H)
    pairs = [node.synth_pair(W, H, 30 + 18 * (b % 4), 900 + b) for b in range(n)]        # scenes at several depths
    Ls = np.stack([p[0] for p in pairs]); Rs = np.stack([p[1] for p in pairs])
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    dD1 = DeviceArray((n, H, W), np.float32); dD2 = DeviceArray((n, H, W), np.float32)
    with jn.Elas(jn.Elas.parameters(0), W, H, max_batch=n) as e:
        assert e.process_batch(n, dL.ptr, dR.ptr, W, H * W, dD1.ptr, dD2.ptr) == [0] * n
    du8 = DeviceArray((n, H, W), np.uint8); bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    node.disparity_scan(sp, n, dD1.ptr, lut.ptr, W, H, du8.ptr, bins.ptr, meta.ptr)
    b_, m_ = bins.numpy(), meta.numpy()
    nav = navigate.Navigator()
    history, last_dir, obstacles = [], 0, 0
    for b in range(n):
        msg = node.laser_scan_message(b_[b], m_[b], seq=b)
        nav.scan_callback(msg)
        d = nav.obstacle_avoid_step()
        _, D1o, _ = oracle.process(oracle.params(0), Ls[b], Rs[b])
        bo, mo, _ = oracle.scan(spo, oracle.to_u8(D1o), luto)
        xy = oracle.scan_to_points(oracle.compact(bo), np.float32(mo[0]), np.float32(mo[1]))
        obst, count, closest, conf = oracle.check_obstacle(xy, history)
        last_dir = oracle.choose_direction(xy, last_dir) if obst else 0
        assert (d["obstacle"], d["points_inside"], d["direction"], d["points"]) == (obst, count, last_dir, len(xy)), b
        assert abs(d["closest"] - closest) <= SCAN_TOL and d["confidence"] == conf
        obstacles += obst
    assert 0 < obstacles


@pytest.mark.parametrize("kind", ["strips", "blobs", "shallow", "patches"])
def test_scan_on_other_scenes(jn, oracle, same, kind):
    """u8 map + LUT + scan (both flavours) on disparity maps with depth jumps inside the 16-row column strips k_scan
    walks, so that bins change within a strip."""
    from scenes import make_scene
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node
    W, H, n = 320, 180, 4
    sp, spo = node.scan_params(W, H), oracle.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    luto = oracle.valid_lut(spo, W, H)
    Ds = []
    for b in range(n):
        L, R = make_scene(kind, W, H, 120, 300 + b)
        _, D1, _ = oracle.process(oracle.params(0, disp_max=127), L, R)
        Ds.append(D1)
    Ds = np.stack(Ds)
    dD = DeviceArray.from_numpy(Ds)
    du8 = DeviceArray((n, H, W), np.uint8); bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
    node.disparity_scan(sp, n, dD.ptr, lut.ptr, W, H, du8.ptr, bins.ptr, meta.ptr)
    bins2 = DeviceArray((n, sp.bins), np.float64); meta2 = DeviceArray((n, 4), np.float64)
    node.obstacle_scan_cloud(sp, n, du8.ptr, W, H, bins2.ptr, meta2.ptr)
    u8, b_, m_, b2, m2 = du8.numpy(), bins.numpy(), meta.numpy(), bins2.numpy(), meta2.numpy()
    for b in range(n):
        u8o = oracle.to_u8(Ds[b])
        assert same(u8[b], u8o)
        bo, mo, _ = oracle.scan(spo, u8o, luto)
        assert np.array_equal(b_[b] < 1e9 - 1, bo < 1e9 - 1)
        assert np.allclose(b_[b], bo, rtol=0, atol=SCAN_TOL) and np.allclose(m_[b], mo, rtol=0, atol=SCAN_TOL)
        bc, mc, _ = oracle.scan_cloud(spo, u8o)
        assert np.array_equal(b2[b] < 1e9 - 1, bc < 1e9 - 1)
        assert np.allclose(b2[b], bc, rtol=0, atol=SCAN_TOL) and np.allclose(m2[b], mc, rtol=0, atol=SCAN_TOL)


def test_fused_submit_scan_equals_separate_calls(jn, same):
    """jn_elas_submit_scan = jn_elas_submit followed by jn_disparity_scan, bit for bit (a failing frame included)."""
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node
    W, H, n = 320, 180, 5
    rng = np.random.default_rng(2)
    Ls = np.stack([node.synth_pair(W, H, 48, 70 + b)[0] for b in range(n)]); Rs = np.stack([node.synth_pair(W, H, 48, 70 + b)[1] for b in range(n)])
    Ls[3] = rng.integers(0, 255, (H, W)); Rs[3] = rng.integers(0, 255, (H, W))          # frame 3 fails
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    outs = []
    with jn.Elas(jn.Elas.parameters(0), W, H, max_batch=n, slots=2) as e:
        for fused in (False, True):
            d1 = DeviceArray.from_numpy(np.zeros((n, H, W), np.float32)); d2 = DeviceArray.from_numpy(np.zeros((n, H, W), np.float32))
            u8 = DeviceArray((n, H, W), np.uint8); bins = DeviceArray((n, sp.bins), np.float64); meta = DeviceArray((n, 4), np.float64)
            st = (C.c_int32 * n)()
            if fused:
                e.submit_scan(1, n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr, sp, lut.ptr, u8.ptr, bins.ptr, meta.ptr, st)
                e.wait(1)
            else:
                e.submit(0, n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr, st)
                e.wait(0)
                node.disparity_scan(sp, n, d1.ptr, lut.ptr, W, H, u8.ptr, bins.ptr, meta.ptr)
            outs.append((list(st), d1.numpy(), d2.numpy(), u8.numpy(), bins.numpy(), meta.numpy()))
    assert outs[0][0] == outs[1][0] == [0, 0, 0, 1, 0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert same(a, b)


def test_scan_with_empty_and_saturated_maps(jn, oracle):
    from jackal_navigation_amd.device import DeviceArray
    from jackal_navigation_amd import node
    W, H = 160, 90
    sp, spo = node.scan_params(W, H), oracle.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    luto = oracle.valid_lut(spo, W, H)
    for fillv in (0, 1, 255):
        disp = np.full((1, H, W), fillv, np.uint8)
        dd = DeviceArray.from_numpy(disp); bins = DeviceArray((1, sp.bins), np.float64); meta = DeviceArray((1, 4), np.float64)
        node.obstacle_scan(sp, 1, dd.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
        bo, mo, used = oracle.scan(spo, disp[0], luto)
        assert np.allclose(bins.numpy()[0], bo, rtol=0, atol=SCAN_TOL), fillv
        assert np.allclose(meta.numpy()[0], mo, rtol=0, atol=SCAN_TOL), fillv


@pytest.mark.parametrize("W,H,sd,dmax,seed,kw", [
    (320, 240, 40, 79, 21, {}), (640, 480, 64, 63, 12345, {"postprocess_only_left": 0}),
    (256, 200, 40, 63, 1, {"filter_median": 1, "postprocess_only_left": 0}),
    (400, 304, 60, 127, 6, {"candidate_stepsize": 4, "ipol_gap_width": 7, "speckle_size": 50, "postprocess_only_left": 0}),
    (322, 182, 48, 255, 12345, {"filter_adaptive_mean": 0}), (1280, 720, 128, 127, 12345, {"postprocess_only_left": 0}),
])
def test_subsampling_gives_the_reference_half_size_maps(jn, oracle, same, W, H, sd, dmax, seed, kw):
    """param.subsampling = 1 (elas.h:82): (W/2) x (H/2) maps, bit-identical to the oracle (which tests/test_oracle_vs_reference.py pins
    against the compiled reference for the same cases).  Through host pointers (jn_elas_process) and through device pointers in a batch
    of two frames of which the second has too few support points (outputs untouched)."""
    import torch
    L, R = jn.node.synth_pair(W, H, sd, seed)
    p = jn.Elas.parameters(0, disp_max=dmax, subsampling=1, **kw)
    st_o, D1o, D2o = oracle.process(oracle.params(0, disp_max=dmax, subsampling=1, **kw), L, R)
    Hh, Wh = H // 2, W // 2
    assert st_o == 0 and D1o.shape == (Hh, Wh)
    D1 = np.full((Hh, Wh), 7.0, np.float32); D2 = np.full((Hh, Wh), 7.0, np.float32)
    with jn.Elas(p, W, H) as e:
        assert e.process(L, R, D1, D2, (W, H, W)) == 0
    assert same(D1, D1o) and same(D2, D2o), (int((D1 != D1o).sum()), int((D2 != D2o).sum()))
    dev = torch.device("cuda", 0)
    flat = np.full((H, W), 128, np.uint8)
    tl = torch.from_numpy(np.stack([L, flat])).to(dev); tr = torch.from_numpy(np.stack([R, flat])).to(dev)
    o1 = torch.full((2, Hh, Wh), -3.0, dtype=torch.float32, device=dev); o2 = torch.full((2, Hh, Wh), -3.0, dtype=torch.float32, device=dev)
    with jn.Elas(p, W, H, max_batch=2, host_threads=4) as e:
        st = e.process_batch(2, tl.data_ptr(), tr.data_ptr(), W, H * W, o1.data_ptr(), o2.data_ptr())
    assert list(st) == [0, 1]
    assert same(o1[0].cpu().numpy(), D1o) and same(o2[0].cpu().numpy(), D2o)
    assert float(o1[1].min()) == -3.0 == float(o1[1].max()) and float(o2[1].min()) == -3.0 == float(o2[1].max())


@pytest.mark.parametrize("fast_max,scan_from", [(16, 64), (3, 64), (0, 64), (3, 6), (0, 0)])
def test_every_ownership_route_gives_the_same_maps(jn, hooks, oracle, same, monkeypatch, fast_max, scan_from):
    """k_owner resolves which triangle owns a pixel three ways: ranked cover words for lists of up to 16 triangles per 32x8 tile (every
    list at 720p so far), the largest covering triangle number entry by entry for longer lists, and a scan over all of a side's triangles
    for tiles whose list overflowed its 64 entries.  The two test hooks lower the thresholds so that ORDINARY lists take the other routes:
    (3, 64) mixes ranked and entry-by-entry, (0, 64) is entry-by-entry only, (3, 6) adds the scan for the longer lists, (0, 0) scans every
    tile.  All of them must give the oracle's maps bit for bit."""
    monkeypatch.setenv("JN_OWNER_FAST_MAX", str(fast_max))
    monkeypatch.setenv("JN_OWNER_SCAN_FROM", str(scan_from))
    from scenes import make_scene
    for kind, W, H, dmax in (("blobs", 320, 240, 79), ("slanted", 333, 201, 63)):
        L, R = make_scene(kind, W, H, dmax, 77)
        p = dict(disp_max=dmax, postprocess_only_left=0)
        st, D1, D2 = run_elas(jn, jn.Elas.parameters(0, **p), L, R)
        st_o, D1o, D2o = oracle.process(oracle.params(0, **p), L, R)
        assert st == st_o == 0 and same(D1, D1o) and same(D2, D2o), (kind, fast_max, scan_from)


def test_natural_image_statistics_take_the_long_list_routes(jn, oracle, same):
    """VERDICT r04 #7c: every input so far was block texture.  The `grain` scene (band-limited noise, film grain, one image defocused) and the
    `periodic` one (bars of period 12) have other statistics; with a support lattice of step 3 nearly every lattice point becomes a support
    point, the triangles get small, and the 32x8 tiles' lists grow past the 16 entries the ownership pass resolves by cover words — asserted
    through jn_elas_bin_stats, not assumed.  D1 / D2 bit for bit against the oracle (which is pinned on these scenes against the compiled
    reference: tests/test_oracle_vs_reference.py, tests/golden/reference_scene_hashes.txt)."""
    from scenes import make_scene
    from jackal_navigation_amd.device import DeviceArray
    took_long = 0
    for kind, W, H, dmax, kw in (("grain", 640, 360, 95, {"candidate_stepsize": 3}), ("periodic", 640, 360, 95, {"candidate_stepsize": 3}),
                                 ("grain", 1280, 720, 127, {}), ("grain", 320, 240, 63, {"candidate_stepsize": 2, "incon_min_support": 3})):
        n = 2
        pairs = [make_scene(kind, W, H, dmax, 90 + b) for b in range(n)]
        Ls = np.stack([p[0] for p in pairs]); Rs = np.stack([p[1] for p in pairs])
        dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
        d1 = DeviceArray((n, H, W), np.float32); d2 = DeviceArray((n, H, W), np.float32)
        p = dict(disp_max=dmax, postprocess_only_left=0, **kw)
        with jn.Elas(jn.Elas.parameters(0, **p), W, H, max_batch=n) as e:
            st = e.process_batch(n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr)
            longest, beyond16, beyond64 = e.bin_stats(0)
        D1, D2 = d1.numpy(), d2.numpy()
        for b in range(n):
            st_o, D1o, D2o = oracle.process(oracle.params(0, **p), Ls[b], Rs[b])
            assert st[b] == st_o == 0 and same(D1[b], D1o) and same(D2[b], D2o), (kind, W, H, b)
        took_long += beyond16
        if kw.get("candidate_stepsize", 5) <= 3:
            assert beyond16 > 0 and longest > 16, (kind, W, H, longest, beyond16)
        for a in (dL, dR, d1, d2):
            a.free()
    assert took_long > 0

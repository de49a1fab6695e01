"""cv::imdecode(GRAYSCALE) restatement (jackal_navigation_amd/csrc/jpeg.hip): the host half on CPU.

Third-party arithmetic (libjpeg via OpenCV) pinned by Pillow / libjpeg-turbo fixtures
(tests/golden/jpeg_cases.npz, tests/golden/make_jpeg_golden.py).  Here: marker parsing and Huffman decoding through the
host hook jn_host_jpeg_coefficients, with the inverse DCT restated in numpy (tests/jpeg_def.py, the IJG "slow integer" definition) so that
the whole chain can be compared with the fixtures without a GPU; tests/test_gpu_round2.py runs the kernel."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import frontend_cases as fc
import jpeg_write
from jpeg_def import decode, islow_idct, range_limit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    return z, names


def host_decode(jn, data):
    L = jn.load()
    buf = np.ascontiguousarray(data, np.uint8)
    q = (C.c_uint16 * 64)()
    w, h, bw, bh = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    n = L.jn_host_jpeg_coefficients(buf.ctypes.data, buf.size, None, 0, q, C.byref(w), C.byref(h), C.byref(bw), C.byref(bh))
    if n < 0:
        return -n, None
    coef = np.zeros(n, np.int16)
    assert L.jn_host_jpeg_coefficients(buf.ctypes.data, buf.size, coef.ctypes.data, n, q, C.byref(w), C.byref(h), C.byref(bw), C.byref(bh)) == n
    quant = np.array(list(q), np.int64).reshape(8, 8)
    blocks = coef.reshape(bh.value, bw.value, 8, 8).astype(np.int64) * quant
    img = np.zeros((bh.value * 8, bw.value * 8), np.uint8)
    for by in range(bh.value):
        for bx in range(bw.value):
            img[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = range_limit(islow_idct(blocks[by, bx], fits_int32=False))   # any file, fuzzed ones too: exact, no condition
    return 0, img[:h.value, :w.value]


def test_entropy_decoder_and_idct_definition_reproduce_libjpeg(jn):
    z, names = cases()
    checked = 0
    for name in names:
        if name == "progressive":
            continue
        st, img = host_decode(jn, z[name + "__jpeg"])
        assert st == 0, name
        assert img.shape == tuple(z[name + "__shape"]), name
        assert hashlib.sha256(img.tobytes()).digest() == z[name + "__sha256"].tobytes(), name
        if name + "__gray" in z.files:
            assert np.array_equal(img, z[name + "__gray"])
        checked += 1
    assert checked >= 10


def test_jpeg_info_and_refusals(jn):
    from jackal_navigation_amd import _lib, node
    z, names = cases()
    assert node.jpeg_info(z["webcam_640x360_q80_420__jpeg"]) == (640, 360)
    assert node.jpeg_info(z["ragged_35x21_q95_422__jpeg"]) == (35, 21)
    with pytest.raises(_lib.JnError) as e:
        node.jpeg_info(z["progressive__jpeg"])
    assert e.value.status == _lib.JN_ERR_UNSUPPORTED
    st, _ = host_decode(jn, z["progressive__jpeg"])
    assert st == _lib.JN_ERR_UNSUPPORTED
    good = z["q90_422__jpeg"]
    for bad in (good[:200], np.zeros(64, np.uint8), good[2:]):
        st, _ = host_decode(jn, bad)
        assert st == _lib.JN_ERR_INVALID
    cut = good[: len(good) // 2].copy()                    # truncated scan: still decodes (zeros are fed past the end), like libjpeg's warning path
    st, img = host_decode(jn, cut)
    assert st in (0, _lib.JN_ERR_INVALID)


def _dht(counts, nsym=None, tc_th=0x00):
    counts = list(counts) + [0] * (16 - len(counts))
    n = sum(counts) if nsym is None else nsym
    body = bytes([tc_th]) + bytes(counts) + bytes(range(n % 257))[:n]
    return b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body


def test_damaged_huffman_tables_and_oversized_frames_are_refused(jn):
    """a DHT that is not a prefix code (255 codes of length 1) made the 8-bit look-up index run past the
    table — an out-of-bounds stack write from a 40-byte file.  libjpeg rejects such tables (JERR_BAD_HUFF_TABLE); so must we.
    (medium): SOF dimensions drive the coefficient buffer; frames beyond 8192x8192 are refused before any allocation."""
    from jackal_navigation_amd import _lib
    soi = b"\xff\xd8"
    for counts in ([255], [3], [2, 3], [1, 1, 1, 1, 1, 1, 1, 1, 2], [0] * 15 + [255, ]):
        st, _ = host_decode(jn, np.frombuffer(soi + _dht(counts) + b"\xff\xd9", np.uint8))
        assert st == _lib.JN_ERR_INVALID, counts
    # the all-ones code of a length is reserved (T.81 C.2): 2 codes of length 1 use it
    st, _ = host_decode(jn, np.frombuffer(soi + _dht([2]) + b"\xff\xd9", np.uint8))
    assert st == _lib.JN_ERR_INVALID
    z, _ = cases()
    good = bytes(z["q90_422__jpeg"])
    i = good.index(b"\xff\xc0")
    huge = bytearray(good); huge[i + 5:i + 9] = b"\xff\xff\xff\xff"          # 65535 x 65535
    st, _ = host_decode(jn, np.frombuffer(bytes(huge), np.uint8))
    assert st == _lib.JN_ERR_UNSUPPORTED
    big = bytearray(good); big[i + 5:i + 9] = (8200).to_bytes(2, "big") + (16).to_bytes(2, "big")
    st, _ = host_decode(jn, np.frombuffer(bytes(big), np.uint8))
    assert st == _lib.JN_ERR_UNSUPPORTED


def test_fuzzed_files_never_crash_the_host_decoder(jn):
    """Small fuzz corpus: byte flips, truncations, spliced segments and random DHT/DQT/SOF/SOS bodies over three valid files.
    Every outcome must be a status (or a decoded image), never a crash; test_sanitizers.py repeats this under ASan/UBSan."""
    z, names = cases()
    rng = np.random.default_rng(2026)
    seeds = [bytes(z[n + "__jpeg"]) for n in ("ragged_35x21_q95_422", "q90_422", "restart_blocks_q80_444")]
    outcomes = {}
    for it in range(600):
        b = bytearray(seeds[it % len(seeds)])
        kind = it % 5
        if kind == 0:                                                       # flips in the headers
            for _ in range(int(rng.integers(1, 8))):
                b[int(rng.integers(2, min(len(b), 700)))] = int(rng.integers(0, 256))
        elif kind == 1:                                                     # flips anywhere
            for _ in range(int(rng.integers(1, 30))):
                b[int(rng.integers(2, len(b)))] = int(rng.integers(0, 256))
        elif kind == 2:
            b = b[:int(rng.integers(2, len(b)))]
        elif kind == 3:                                                     # a random table segment right after SOI
            m = [0xC4, 0xDB, 0xC0, 0xDA, 0xDD][int(rng.integers(0, 5))]
            body = bytes(rng.integers(0, 256, int(rng.integers(0, 300))).astype(np.uint8))
            b = bytearray(b[:2] + bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + body + bytes(b[2:]))
        else:                                                               # a random prefix-violating DHT
            b = bytearray(b[:2] + _dht(list(rng.integers(0, 256, 16)), nsym=int(rng.integers(0, 257))) + bytes(b[2:]))
        st, img = host_decode(jn, np.frombuffer(bytes(b), np.uint8))
        outcomes[st] = outcomes.get(st, 0) + 1
    assert set(outcomes) <= {0, 2, 3, 5}, outcomes
    assert outcomes.get(3, 0) > 50, outcomes


def host_coefficients(jn, data):
    L = jn.load()
    buf = np.frombuffer(bytes(data), np.uint8)
    q = (C.c_uint16 * 64)()
    w, h, bw, bh = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    n = L.jn_host_jpeg_coefficients(buf.ctypes.data, buf.size, None, 0, q, C.byref(w), C.byref(h), C.byref(bw), C.byref(bh))
    assert n == bw.value * bh.value * 64, n
    coef = np.zeros(n, np.int16)
    assert L.jn_host_jpeg_coefficients(buf.ctypes.data, buf.size, coef.ctypes.data, n, q, C.byref(w), C.byref(h), C.byref(bw), C.byref(bh)) == n
    return coef.reshape(bh.value, bw.value, 8, 8), np.array(list(q)).reshape(8, 8), w.value, h.value


def test_written_coefficients_come_back_from_the_entropy_decoder(jn):
    """tests/jpeg_write.py -> jn_host_jpeg_coefficients: exactly the coefficients, the table and the frame size that were written, for
    every synthetic frame of frontend_cases.jpeg_frames (the frames tests/test_gpu_frontend.py hands to the GPU's inverse DCT)."""
    frames = fc.jpeg_frames()
    assert {(W, H) for _, W, H, _, _, _ in frames} == set(fc.JPEG_SIZES)
    for name, W, H, quant, coef, _ in frames:
        got, q, w, h = host_coefficients(jn, jpeg_write.write_gray(coef, quant, W, H))
        assert (w, h) == (W, H), name
        assert np.array_equal(q, quant), name
        assert np.array_equal(got, coef), name


def test_synthetic_blocks_reach_every_branch_of_the_range_limit_within_int32():
    """The reference alone, on the CPU.  Every block of the q1 and dense pools passes jpeg_def's int32 assertion (none is dropped);
    every block of the q255 pool fails it (1023 * 255 needs more than 32 bits at every position, frontend_cases.jpeg_pools).
    The dense pool spreads past +-1500 before range limiting, and over all pools each of range_limit's four branches and the wrap
    beyond +512 and beyond -512 (where the table's answer is not the clamp's) is hit."""
    pre = {}
    for name, quant, blocks, fits in fc.jpeg_pools():
        if fits:
            pre[name] = np.array([islow_idct(b * quant) for b in blocks])                 # asserts int32 for each block
        else:
            pre[name] = np.array([islow_idct(b * quant, fits_int32=False) for b in blocks])
            for b in blocks[6:]:                                                          # the singles (the first six are DC alone)
                with pytest.raises(AssertionError):
                    islow_idct(b * quant)
    assert pre["dense"].min() <= -1500 and pre["dense"].max() >= 1500
    assert np.percentile(pre["dense"], 5) < -1500 and np.percentile(pre["dense"], 95) > 1500    # spread, not two outliers
    x = np.concatenate([p.ravel() for p in pre.values()])
    i = x & 1023
    for hit in (i < 128, (i >= 128) & (i < 512), (i >= 512) & (i < 896), i >= 896):
        assert hit.any()
    d = pre["dense"].ravel()                                      # the wrap is reached by blocks that fit int32, not by q255 alone
    clamp = np.clip(d + 128, 0, 255)
    for beyond in (d >= 512, d < -512):
        assert (range_limit(d)[beyond] != clamp[beyond]).any()


def test_pillow_decodes_written_files_like_the_definition(jn):
    """When Pillow imports: libjpeg-turbo's decode of a written file equals jpeg_def for blocks whose dequantised values stay within
    +-1024 and whose results stay within the range table's unwrapped span (-512 <= x < 512; two coefficients per block keep them
    there: 2 * 1024 * 0.2405 < 512).  Extreme blocks are not pinned against it: its SIMD inverse DCT works in 16 bits and
    saturates where the table wraps."""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(8)
    peak = 0
    for k, (W, H) in enumerate(fc.JPEG_SIZES + ((35, 21),)):
        bw, bh = (W + 7) // 8, (H + 7) // 8
        quant = rng.integers(1, 17, (8, 8))
        coef = np.zeros((bh * bw, 64), np.int64)
        for b in coef:
            for pos in rng.integers(0, 64, 2):
                b[pos] = rng.integers(-1024, 1025) // quant.ravel()[pos]
        coef = coef.reshape(bh, bw, 8, 8)
        assert np.abs(coef * quant).max() <= 1024 and np.abs(decode(coef, quant, W, H)[1]).max() < 512
        peak = max(peak, np.abs(coef * quant).max())
        data = jpeg_write.write_gray(coef, quant, W, H)
        im = Image.open(io.BytesIO(data)); im.load()
        assert im.mode == "L" and im.size == (W, H)
        img, _ = decode(coef, quant, W, H)
        assert np.array_equal(np.asarray(im), img), (W, H)
        st, ours = host_decode(jn, np.frombuffer(data, np.uint8))
        assert st == 0 and np.array_equal(ours, img)
    assert peak > 1000

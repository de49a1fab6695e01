"""A minimal baseline JPEG writer for tests: one grey component, SOF0, the luminance Huffman tables of ITU-T T.81 Annex K (K.3, K.5),
an arbitrary 8-bit quantisation table, byte stuffing.  It turns given QUANTISED coefficients into a file, so that a test chooses
what the inverse DCT sees.  TEST INFRASTRUCTURE.  The tables limit a DC difference to 11 bits and an AC coefficient to 10."""
import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
DC_COUNTS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_VALUES = tuple(range(12))
AC_COUNTS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)
AC_VALUES = bytes.fromhex(
    "0102030004110512" "2131410613516107" "227114328191a108" "2342b1c11552d1f0" "2433627282090a16" "1718191a25262728"
    "292a343536373839" "3a43444546474849" "4a53545556575859" "5a63646566676869" "6a73747576777879" "7a83848586878889"
    "8a92939495969798" "999aa2a3a4a5a6a7" "a8a9aab2b3b4b5b6" "b7b8b9bac2c3c4c5" "c6c7c8c9cad2d3d4" "d5d6d7d8d9dae1e2"
    "e3e4e5e6e7e8e9ea" "f1f2f3f4f5f6f7f8" "f9fa")


def _codes(counts, values):
    """symbol -> (code, length): T.81 Annex C, codes of one length are consecutive, the next length continues at twice the value."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[values[k]] = (code, length)
            code += 1; k += 1
        code <<= 1
    return out


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def write_gray(coef, quant, width, height):
    """coef [bh][bw][8][8] quantised coefficients ([row][col] = [vertical][horizontal] frequency), bh = ceil(height / 8),
    bw = ceil(width / 8); quant [8][8] in 1..255.  -> the bytes of a baseline JPEG file."""
    coef = np.asarray(coef).astype(np.int64)
    quant = np.asarray(quant).astype(np.int64).reshape(64)
    bh, bw = (height + 7) // 8, (width + 7) // 8
    assert coef.shape == (bh, bw, 8, 8) and quant.min() >= 1 and quant.max() <= 255
    dc, ac = _codes(DC_COUNTS, DC_VALUES), _codes(AC_COUNTS, AC_VALUES)
    acc, nbits = 0, 0                                         # the entropy-coded segment as one big integer

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code; nbits += length

    def put_value(v, size):                                   # T.81 F.1.2.1: negative values as v - 1 in `size` bits
        if size:
            put(v if v > 0 else v + (1 << size) - 1, size)

    pred = 0
    for blk in coef.reshape(-1, 64):
        diff = int(blk[0]) - pred; pred = int(blk[0])
        size = abs(diff).bit_length()
        assert size <= 11, "DC difference %d needs more than 11 bits" % diff
        put(*dc[size]); put_value(diff, size)
        run = 0
        for k in range(1, 64):
            v = int(blk[ZIGZAG[k]])
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ac[0xF0]); run -= 16
            size = abs(v).bit_length()
            assert size <= 10, "AC coefficient %d needs more than 10 bits" % v
            put(*ac[(run << 4) | size]); put_value(v, size)
            run = 0
        if run:
            put(*ac[0x00])
    pad = -nbits % 8
    put((1 << pad) - 1, pad)                                  # fill the last byte with ones
    scan = acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00")
    out = b"\xff\xd8"
    out += _segment(0xDB, bytes([0]) + bytes(int(quant[z]) for z in ZIGZAG))
    out += _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([1, 1, 0x11, 0]))
    out += _segment(0xC4, bytes([0x00]) + bytes(DC_COUNTS) + bytes(DC_VALUES))
    out += _segment(0xC4, bytes([0x10]) + bytes(AC_COUNTS) + AC_VALUES)
    out += _segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    return out + scan + b"\xff\xd9"

"""The IJG "slow integer" inverse DCT and sample range limit, restated in int64 numpy (exact): the reference of tests/test_jpeg.py
and tests/test_gpu_frontend.py for k_jpeg_idct_gray (csrc/jpeg.hip).  TEST INFRASTRUCTURE.

libjpeg forms these sums in a C `long` (INT32 / JLONG), 64 bits wide on every LP64 host, stores the pass-1 workspace as `int`
(a conversion that keeps the low 32 bits) and masks the final value with & 1023.  `islow_idct` does the same: int64 sums, the
workspace wrapped to int32, so its result is libjpeg's for any dequantised block.  A kernel that forms the sums in 32 bits agrees with
it only while they fit; `islow_idct` therefore asserts by default that every intermediate fits int32, and a caller whose block
cannot (see frontend_cases.jpeg_pools) says so with fits_int32=False."""
import numpy as np

I32 = 2 ** 31


def _one_d(v, shift, seen):
    def keep(*xs):
        for x in xs if seen is not None else ():
            seen.append(np.abs(x).max())
        return xs if len(xs) > 1 else xs[0]
    z2, z3 = v[2], v[6]
    z1 = keep((z2 + z3) * 4433)
    tmp2, tmp3 = keep(z1 + z3 * (-15137), z1 + z2 * 6270)
    tmp0, tmp1 = keep((v[0] + v[4]) << 13, (v[0] - v[4]) << 13)
    tmp10, tmp13, tmp11, tmp12 = keep(tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2)
    t0, t1, t2, t3 = v[7], v[5], v[3], v[1]
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; z4 = t1 + t3
    z5 = keep((z3 + z4) * 9633)
    t0, t1, t2, t3 = keep(t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299)
    z1, z2 = keep(z1 * -7373, z2 * -20995)
    z3, z4 = keep(z3 * -16069, z4 * -3196)
    z3, z4 = keep(z3 + z5, z4 + z5)
    keep(z1 + z3, z2 + z4, z2 + z3, z1 + z4, t0 + z1, t1 + z2, t2 + z2, t3 + z1)      # the partial sums, in either order of evaluation
    t0, t1, t2, t3 = keep(t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4)
    r = 1 << (shift - 1)
    sums = keep(tmp10 + t3 + r, tmp11 + t2 + r, tmp12 + t1 + r, tmp13 + t0 + r, tmp13 - t0 + r, tmp12 - t1 + r, tmp11 - t2 + r, tmp10 - t3 + r)
    keep(tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3)
    return [s >> shift for s in sums]


def islow_idct(block, fits_int32=True):
    """8x8 inverse DCT of one DEQUANTISED block [row][col] (CONST_BITS 13, PASS1_BITS 2), result before range limiting.
    fits_int32=True asserts that no intermediate of either pass leaves int32."""
    b = np.asarray(block).astype(np.int64)
    seen = [np.abs(b).max()] if fits_int32 else None
    ws = np.stack(_one_d([b[r] for r in range(8)], 11, seen))             # pass 1 works on columns: element r of every column at once
    ws = ((ws + I32) & (2 * I32 - 1)) - I32                                  # `int workspace[]`: the low 32 bits, signed
    out = np.stack(_one_d([ws[:, k] for k in range(8)], 18, seen), axis=1)
    if fits_int32:
        assert max(seen) < I32, "an intermediate of this block needs more than 32 bits (%d)" % max(seen)
    return out


def range_limit(x):
    """IJG sample range table, indexed modulo 1024 around +128: four branches, and values beyond +-512 WRAP (no clamp)."""
    i = np.asarray(x) & 1023
    return np.where(i < 128, 128 + i, np.where(i < 512, 255, np.where(i < 896, 0, i - 896))).astype(np.uint8)


def decode(coef, quant, width, height, fits_int32=True):
    """coef [bh][bw][8][8] quantised, quant [8][8] -> (grey image [height][width], the values before range limiting [8 bh][8 bw])."""
    coef = np.asarray(coef, np.int64)
    bh, bw = coef.shape[:2]
    pre = np.zeros((bh * 8, bw * 8), np.int64)
    for by in range(bh):
        for bx in range(bw):
            pre[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = islow_idct(coef[by, bx] * np.asarray(quant, np.int64).reshape(8, 8), fits_int32)
    return range_limit(pre)[:height, :width], pre

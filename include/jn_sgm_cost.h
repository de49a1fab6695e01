/* jn_sgm_cost.h — a byte cost volume as an input of the SGM mode's sweeps (jn_sgm.h), and its two producers: the block-SSD
 * cost from the matrix cores and the census / Hamming cost.  C ABI of libjn_stereo.so.
 *
 * NO REFERENCE COUNTERPART (like jn_sgm.h and jn_bm.h): the mode is defined HERE and restated scalar in
 * tests/sgm_cost_def.py (numpy, the checker): parity is SELF-REFERENTIAL ("parity unpinned").  The
 * restatement is anchored to the two definitions it joins: fed jn_sgm.h's 1x3 SAD as its volume, its aggregation equals
 * oracle/sgm_oracle.cpp bit for bit, and its SSD equals a literal triple loop.
 *
 * Definition (all integer).  g, cl, cr, D, P1, P2, the 8 paths, the sum S, WTA, the right image's winners, the L/R
 * check, the sub-pixel step and the output are jn_sgm.h's, word for word; only C(x,y,d) differs:
 *   SSD_r(x,y,d) = sum_{j=-r..r} sum_{i=-r..r} ( gL(cl(x+i), cr(y+j)) - gR(cl(x+i-d), cr(y+j)) )^2
 *                  (jn_bm.h's CL with JN_BM_COST_SSD; cr = clamp to [0, H-1])
 *   C(x,y,d)     = min( SSD_r(x,y,d) >> cost_shift, cost_max )
 * with r in {2, 3, 4}, 0 <= cost_shift <= 12, 1 <= cost_max and cost_max + P2 <= 255, so that every L_r still fits a
 * byte-sized excess and S 16 bits (jn_sgm.h's rule with cost_max in place of 3*2*cap).  D is 64, 128 or 256.
 * This is BASELINE.json config 5's "int8 cost volume (CDNA4 MFMA path)" under the 8-path aggregation: what other
 * libraries call the block size of a semi-global block matcher.
 *
 * JN_SGM_COST_CENSUS: the census transform with a Hamming distance, on the RAW u8 images (no Sobel prefilter; prefilter_cap is
 * range-checked as for the other costs and otherwise unused).  All integer:
 *   window       r = block_radius in {2, 3, 4}: rx = r, ry = min(r, 3)  ->  5x5 (24 bits), 7x7 (48 bits), 9x7 (62 bits)
 *   cen_I(x,y)   = the set of (i,j) != (0,0), |i| <= rx, |j| <= ry, with I(cl(x+i), cr(y+j)) < I(x,y)   (strictly less)
 *   Hm(x,y,d)    = | cen_L(x,y)  symmetric-difference  cen_R(cl(x-d), y) |   (the CENTRE column is clamped, then its window)
 *   C(x,y,d)     = min( Hm(x,y,d), cost_max ),  1 <= cost_max, cost_max + P2 <= 255;  cost_shift is ignored
 * Only Hamming distances are observable: the bit order of a signature is the implementation's business, not the ABI's.
 * Why: the rig is two separately exposed cameras (own auto-exposure and white balance each).  The Sobel prefilter of the
 * other two costs removes an offset between the eyes, not a gain or a gamma; a census signature depends on the ORDER of
 * the grey values in its window only, so any strictly increasing change of one eye's grey scale leaves every C untouched.
 * Like everything here it has no reference counterpart and its parity is self-referential (tests/sgm_census_def.py, anchored
 * to a literal loop).  DEFAULTS UNTUNED: with a 62-bit census P2 = 60 is the whole cost range; other libraries pair a 9x7
 * census with a P2 around 100-120.  Nobody here has measured which is better, and no accuracy comparison of the three costs
 * exists (every input in this tree is synthetic).
 *
 * With JN_SGM_COST_EXTERNAL the caller brings C itself: a volume [n][H][W][D] of bytes, natural column order, d
 * ascending, every byte <= 255 - P2 (not checked), and the handle only aggregates it.
 *
 * Defaults: r = 2, cost_shift = 5, cost_max = 127 (with jn_sgm.h's P1 = 10, P2 = 60).  A 5x5 SSD of two unrelated
 * patches at cap = 31 is a few 10^4; >> 5 puts a one-grey-level-per-pixel mismatch (25) below 1 and saturates at
 * SSD = 4096, about 13 grey levels per pixel, which keeps P2 = 60 roughly half of the cost range as it is for the
 * 1x3 SAD.  Nobody has measured which values give the best maps: these are a starting point, not a tuning result.
 */
#ifndef JN_SGM_COST_H
#define JN_SGM_COST_H

#include <stdint.h>
#include "jn_sgm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jn_sgm_cost_params {
  int32_t cost_function;   /* JN_SGM_COST_* */
  int32_t block_radius;    /* r: 2, 3 or 4 (BLOCK_SSD: the block; CENSUS: the window 5x5, 7x7, 9x7; ignored otherwise) */
  int32_t cost_shift;      /* 0..12 (BLOCK_SSD; ignored otherwise) */
  int32_t cost_max;        /* 1..255 - P2 (BLOCK_SSD, CENSUS) */
} jn_sgm_cost_params;
#define JN_SGM_COST_SAD3      0   /* jn_sgm.h's cost: jn_sgm_create_cost then behaves exactly like jn_sgm_create */
#define JN_SGM_COST_BLOCK_SSD 1
#define JN_SGM_COST_EXTERNAL  2   /* the handle only aggregates volumes the caller brings (P2 <= 254) */
#define JN_SGM_COST_CENSUS    4   /* not 3: 3 is no cost function and stays refused, as it always was */

/* BLOCK_SSD, r = 2, cost_shift = 5, cost_max = 127 */
void jn_sgm_cost_params_default(jn_sgm_cost_params* c);

/* A jn_sgm handle with the given cost.  On a BLOCK_SSD or CENSUS handle jn_sgm_process_batch, jn_sgm_submit_scan / jn_sgm_wait
 * (all slots), jn_sgm_last_times (prefilter includes the producer), the attached post-filter and the navigation
 * tails run that cost with no further API; each slot then holds one more byte volume of max_batch*W*H*D
 * (CENSUS: and 16 bytes of signatures per pixel pair), allocated when the slot is first used.  JN_ERR_UNSUPPORTED for what
 * lies outside the ranges above. */
jn_status jn_sgm_create_cost(const jn_sgm_params* p, const jn_sgm_cost_params* c, int32_t width, int32_t height, int32_t max_batch,
                             int32_t device, jn_sgm** out);

/* Producer only (BLOCK_SSD and CENSUS handles; JN_ERR_UNSUPPORTED on others): the cost volume of n pairs, dCost [n][H][W][D] u8
 * (device, 16-byte aligned; natural column order, d ascending).  Synchronous. */
jn_status jn_sgm_cost_volume(jn_sgm* h, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch, int64_t image_stride,
                             uint8_t* dCost);

/* Consumer only (BLOCK_SSD, CENSUS and EXTERNAL handles): 8 paths + WTA + L/R + sub-pixel over a caller's volume (16-byte
 * aligned, every byte <= 255 - P2, not checked) -> dDisp [n][H][W] int16.  Synchronous.
 * On an EXTERNAL handle the calls that take images return JN_ERR_UNSUPPORTED. */
jn_status jn_sgm_aggregate_batch(jn_sgm* h, int32_t n, const uint8_t* dCost, int16_t* dDisp);

#ifdef __cplusplus
}
#endif
#endif /* JN_SGM_COST_H */

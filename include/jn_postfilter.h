/* jn_postfilter.h — C ABI of the disparity post-filter of libjn_stereo.so: speckle removal by connected components, then an optional
 * 3x3 median, for the int16 maps of the SGM and block-matching modes (jn_sgm.h, jn_bm.h).
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation's only matcher is libelas, which cleans its own float map (L/R check, speckle
 * removal, gap interpolation, adaptive mean, median: elas.cpp:981-1099 and on); the SGM and block-matching modes of this library stop
 * at the L/R check.  The obstacle scan keeps the SMALLEST range per bin (jn_obstacle_scan, jn_subpix_scan), so a surviving mismatch of
 * a handful of pixels at a large disparity is a phantom obstacle in front of a far wall.  This filter is what OpenCV's StereoBM /
 * StereoSGBM users know as speckleWindowSize / speckleRange plus a median.  Like jn_costmap.h, jn_ground.h and jn_subpix.h it is
 * defined HERE: parity is SELF-REFERENTIAL, its scalar restatement (the checker) lives in the tests (tests/postfilter_def.py), and the
 * bar is bit-identity with it.
 *
 * Definition (all integer arithmetic; no result depends on the order pixels are visited in).
 *   input          n maps [n][height][width] int16 on the device, in one of jn_subpix.h's formats
 *                    JN_DISP_I16      integer pixels
 *                    JN_DISP_I16_SUB  1/16 pixel
 *                  JN_DISP_F32 is refused (ELAS filters its own map).  Frames are independent: nothing connects the last row of one
 *                  map to the first row of the next.
 *   valid          a pixel whose value v >= 0.  Its disparity in 1/16 pixel is q = 16 v (I16) or q = v (I16_SUB), as jn_subpix.h
 *                  defines q.
 *   1 speckles     (speckle_size >= 1; 0 skips the stage.)  Take the graph whose nodes are the valid pixels of one map and whose edges
 *                  join 4-neighbours p, p' with |q(p) - q(p')| <= speckle_range_q.  Its connected components are the SEGMENTS (the
 *                  relation is closed transitively: a ramp 0, 1, 2, ... with a range of one pixel is ONE segment).  A segment with
 *                  FEWER THAN speckle_size pixels is a speckle; all its pixels become invalid.
 *   2 median       (median = 1; 0 skips the stage.)  On stage 1's output, not in place: for every valid pixel take the values of the
 *                  valid pixels of its 3x3 window clipped to the image (k of them, 1 <= k <= 9, the centre among them), sort them
 *                  ascending, and output element (k - 1) / 2 (integer division: the lower median).  Invalid pixels stay invalid;
 *                  nothing is filled in.
 *   output         int16 in the input's format.  A pixel that was invalid on input is copied unchanged; a pixel stage 1 invalidated
 *                  gets the matchers' marker, -1 (I16) or -16 (I16_SUB).  dOut == dIn is allowed.
 *   statistics     (optional) dStats [n][4] uint32 per map: valid pixels on input, segments, speckle segments, pixels removed.  With
 *                  speckle_size = 0 no segments are formed and the last three are 0.
 */
#ifndef JN_POSTFILTER_H
#define JN_POSTFILTER_H

#include <stdint.h>
#include "jn_stereo.h"
#include "jn_subpix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_POSTFILTER_MAX_SIDE 8192
#define JN_POSTFILTER_MAX_SPECKLE_SIZE (1 << 24)
#define JN_POSTFILTER_MAX_RANGE_Q 4096

typedef struct jn_postfilter_params {
  int32_t format;              /* jn_disp_format: JN_DISP_I16 or JN_DISP_I16_SUB */
  int32_t speckle_size;        /* segments with fewer pixels are removed, [0, JN_POSTFILTER_MAX_SPECKLE_SIZE]; 0: no speckle stage */
  int32_t speckle_range_q;     /* largest step between 4-neighbours of one segment, in 1/16 pixel, [0, JN_POSTFILTER_MAX_RANGE_Q] */
  int32_t median;              /* 0 or 1 */
} jn_postfilter_params;

/* speckle_size = 200 (libelas' own preset, elas.h:92-115), speckle_range_q = 16 (one pixel), median = 0 */
void jn_postfilter_params_default(jn_postfilter_params* fp, int32_t format);

/* Synchronous; device pointers.  Argument errors — a NULL fp / dIn / dOut, n < 1, width or height outside [1, JN_POSTFILTER_MAX_SIDE],
 * an unknown format or JN_DISP_F32, a field of fp outside its range — return JN_ERR_INVALID before the device is touched; without a
 * device the call returns JN_ERR_NO_DEVICE.  dStats may be NULL.  The labels live in the calling thread's grow-only device scratch
 * (8 bytes per pixel; 2 more for an in-place median). */
jn_status jn_disparity_postfilter(int32_t device, const jn_postfilter_params* fp, int32_t n, const int16_t* dIn, int32_t width,
                                  int32_t height, int16_t* dOut, uint32_t* dStats);

/* The filter as part of an SGM slot's batch.  From this call on EVERY batch submitted on `slot` (jn_sgm_submit_scan with or without scan
 * parameters) is filtered in place in the caller's dDisp, on the slot's stream: sweeps, L/R check into dDisp, the filter, then — with scan
 * parameters — the mono8 map OF THE FILTERED MAP, the LUT scan, an attached jn_costmap, an attached sub-pixel tail.  Every consumer sees
 * filtered data and nothing synchronises with the host in between.  (The one-kernel tail that applies the L/R check and scans at once
 * cannot sit behind a filter; such a slot queues the L/R check, jn_sgm_disparity_to_u8's kernel and the scan one after the other.)
 * fp->format must be the handle's own format (JN_DISP_I16_SUB iff it was created with subpixel = 1), else JN_ERR_INVALID.
 * dStats [max_batch][4] or NULL, valid after the slot's wait.  fp == NULL detaches.  Call with no batch in flight on the slot.  A slot with
 * nothing attached queues exactly what it queued before this header existed.
 *
 * The block matcher (jn_bm.h) has no attach call.  Its recipe: jn_bm_submit_scan(..., sp = NULL, ...) and jn_bm_wait, then
 *   jn_disparity_postfilter(device, &fp, n, dDisp, W, H, dDisp, dStats);                    in place on the slot's map
 *   jn_sgm_disparity_to_u8(device, dDisp, subpixel, dDispU8, n * W * H);  jn_obstacle_scan(device, &sp, n, dDispU8, dLut, W, H, dBins, dMeta);
 * or jn_subpix_costmap(device, &sp, &cp, &sfp, n, dDisp, W, H, ...) for the sub-pixel scan and grid of the filtered map. */
struct jn_sgm;
jn_status jn_sgm_attach_postfilter(struct jn_sgm* h, int32_t slot, const jn_postfilter_params* fp, uint32_t* dStats);

#ifdef __cplusplus
}
#endif
#endif /* JN_POSTFILTER_H */

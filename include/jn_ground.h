/* jn_ground.h — C ABI of the ground-plane estimator of libjn_stereo.so: the camera-to-robot transform (XR / XT of jn_scan_params) from
 * the floor in a disparity map.
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation gets XR / XT by hand (README step 3: identity and zero, `point_cloud -g -m`, six
 * rqt_reconfigure sliders turned until the cloud's ground "visually aligns" in rviz, the printed matrices copied into the calibration
 * file).  This mode is therefore defined HERE, like jn_sgm.h and jn_costmap.h; its scalar restatement (the checker) lives in the tests
 * (tests/ground_def.py).  Everything the device computes is INTEGER arithmetic: independent of the order pixels are visited in and of
 * FMA contraction, so the bar for it is bit-identity.
 *
 * Definition.  A plane in the camera frame is a plane in (x, y, d); it is fitted there, where the matcher's noise is uniform.
 *   input        n maps [n][height][width] on the device, width and height in [1, JN_GROUND_MAX_SIDE], in one of
 *                  JN_GROUND_F32      float, pixels (ELAS's D1)
 *                  JN_GROUND_I16      int16, integer pixels (SGM / block matching)
 *                  JN_GROUND_I16_SUB  int16, 1/16 pixel (SGM / block matching with sub-pixel interpolation)
 *   q            every pixel's disparity in 1/16 pixel, int32.  F32: t = rint(16 * d) in float (round half to even; 16 * d is exact),
 *                q = t; a non-finite d is invalid.  I16: q = 16 * d.  I16_SUB: q = d.
 *   valid        16 * min_disp <= q <= 16 * JN_GROUND_MAX_SIDE (F32: the same comparison on t before the conversion).  The upper bound
 *                (no disparity exceeds the frame's width) is what keeps the plane coefficients below in int32.
 *   region       the pixels roi_x0 <= x < roi_x1, roi_y0 <= y < roi_y1; roi_w = roi_x1 - roi_x0, roi_h = roi_y1 - roi_y0.
 *   mix32(x)     on uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   hypotheses   K = `hypotheses` per frame.  Point j in {0, 1, 2} of hypothesis k of frame f is looked for in attempts t = 0..7:
 *                  h = mix32(seed ^ mix32((((f * 1024 + k) * 3 + j) * 8) + t))                         (uint32, wrapping)
 *                  x = roi_x0 + (((h & 0xffff) * roi_w) >> 16),   y = roi_y0 + (((h >> 16) * roi_h) >> 16)
 *                the first attempt that lands on a valid pixel is the point (x, y, q); if none does the hypothesis is VOID.
 *                (A, B, C) = (p1 - p0) x (p2 - p0) on (x, y, q), E = -(A x0 + B y0 + C q0): the plane A x + B y + C q + E = 0.
 *                |A|, |B|, |C| < 2^31 and E fits int64.  VOID also if C == 0 or if the plane fails the ground gate
 *                  -B / C >= 16 * beta_min      (disparity grows down the image: a floor, not a ceiling or a facing wall)
 *                  |A / C| <= 16 * alpha_max    (no side walls)
 *                evaluated exactly in int64 with the limits converted once to Q16, bq = llrint(16 * beta_min * 65536),
 *                aq = llrint(16 * alpha_max * 65536):   -B * sign(C) * 65536 >= bq * |C|   and   |A| * 65536 <= aq * |C|.
 *   score        inliers[f][k] = number of valid region pixels with |A x + B y + C q + E| <= tol_q * |C| (int64).  VOID hypotheses
 *                score 0.  The winner `best` is the largest count, on a tie the smallest k.
 *   refit sums   over the winner's inliers (none when the winner is VOID), int64, in this order:
 *                  N, Sx, Sy, Sq, Sxx, Sxy, Syy, Sxq, Syq, Sqq          (x, y frame coordinates, q as above)
 *                and `valid`, the number of valid region pixels.
 *   plane        (host, double) the least-squares plane of the inliers from the centred normal equations.  With the exact integers
 *                Mab = N Sab - Sa Sb converted to double:  det = Mxx Myy - Mxy Mxy,
 *                  aq = (Mxq Myy - Myq Mxy) / det,  bq = (Myq Mxx - Mxq Mxy) / det,  cq = (Sq - aq Sx - bq Sy) / N,
 *                  a, b, c = aq / 16, bq / 16, cq / 16  (d = a x + b y + c in pixels),  rms = sqrt(max(0, Mqq - aq Mxq - bq Myq)) / N / 16.
 *   status       JN_ERR_FEW_SUPPORT when N < 3, N < min_inliers, N < min_inlier_frac * valid or det <= 0 (plane and geometry are then
 *                zero), else JN_OK.
 *   geometry     through Q and the crop offsets of the jn_scan_params:  pi_d = (a, b, -1, c - a crop_offset_x - b crop_offset_y) is the
 *                plane on [x + crop_offset_x, y + crop_offset_y, d, 1];  pi_3 = Q^-T pi_d, divided by the length of its first three entries
 *                and signed so that the camera origin is on its positive side:  n_cam = pi_3[0..2] (unit, from the floor towards the
 *                camera), height_m = pi_3[3] > 0.
 *
 * What a plane fixes: roll, pitch and height.  Yaw and the horizontal offset XT.x / XT.y are NOT observable from a floor and stay the
 * prior's.
 */
#ifndef JN_GROUND_H
#define JN_GROUND_H

#include <stdint.h>
#include "jn_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_GROUND_MAX_SIDE 4096          /* width, height, and the largest valid disparity in pixels */
#define JN_GROUND_MAX_HYPOTHESES 1024

typedef enum jn_ground_format { JN_GROUND_F32 = 0, JN_GROUND_I16 = 1, JN_GROUND_I16_SUB = 2 } jn_ground_format;

typedef struct jn_ground_params {
  int32_t roi_x0, roi_y0, roi_x1, roi_y1;   /* 0 <= x0 < x1 <= width, 0 <= y0 < y1 <= height */
  int32_t hypotheses;                       /* K: a multiple of 64 in [64, 1024] */
  int32_t tol_q;                            /* inlier band in 1/16 pixel, [0, 65536] */
  int32_t min_disp;                         /* pixels, [0, 4096] */
  int32_t min_inliers;                      /* >= 0 */
  uint32_t seed;
  int32_t reserved;                         /* 0 */
  double min_inlier_frac;                   /* [0, 1] */
  double beta_min;                          /* pixels of disparity per row, |beta_min| <= 64 */
  double alpha_max;                         /* pixels of disparity per column, [0, 64] */
} jn_ground_params;

typedef struct jn_ground_plane {
  int32_t status;              /* JN_OK or JN_ERR_FEW_SUPPORT */
  int32_t best;                /* the winning hypothesis */
  int64_t inliers;             /* its score (== sums[0]) */
  int64_t valid;               /* valid region pixels */
  int64_t sums[10];            /* N Sx Sy Sq Sxx Sxy Syy Sxq Syq Sqq */
  double a, b, c, rms;         /* d = a x + b y + c, pixels */
  double n_cam[3], height_m;
} jn_ground_plane;

/* the lower half of the frame at full width, K = 256, tol_q = 8 (half a pixel), min_disp 1, min_inliers 500, seed 0x9e3779b9,
 * min_inlier_frac 0.2, beta_min 0.02, alpha_max 0.25 */
void jn_ground_params_default(jn_ground_params* gp, int32_t width, int32_t height);

/* n maps dDisp [n][height][width] (device, `format`) -> out[n] (host).  scores [n][K] int32 and hyps [n][K][4] int64 (A, B, C, E; all
 * zero for a VOID hypothesis) are optional host arrays.  sp supplies Q and the crop offsets (its XR / XT are not read).  Synchronous.
 * Argument errors (NULL sp / gp / dDisp / out, n outside [1, 65535], width or height outside [1, 4096], an unknown format, an empty or out-of-frame
 * region, K not a multiple of 64 in [64, 1024], any other field outside the range given above, a singular Q) return JN_ERR_INVALID
 * before the device is touched; without a device the call returns JN_ERR_NO_DEVICE. */
jn_status jn_ground_estimate(int32_t device, const jn_scan_params* sp, const jn_ground_params* gp, int32_t n, const void* dDisp,
                             int32_t format, int32_t width, int32_t height, jn_ground_plane* out, int32_t* scores, int64_t* hyps);

/* Host only: the plane, status and geometry of `sums` / `valid` by the rules above (what jn_ground_estimate does per frame after the
 * device pass; `best` and `inliers` are set to 0 and sums[0]).  gp supplies min_inliers / min_inlier_frac. */
jn_status jn_ground_solve(const jn_scan_params* sp, const jn_ground_params* gp, const int64_t sums[10], int64_t valid, jn_ground_plane* out);

/* The prior for a rig that has none: a forward-looking camera, robot x = camera z, robot y = -camera x, robot z = -camera y:
 * XR = [0 0 1; -1 0 0; 0 -1 0], XT = 0.  (The README's starting point, identity and zero, cannot serve: its up direction is the optical
 * axis, 90 degrees from any floor.)  The shipped rig's XR is 15.5 degrees of pitch away from this one. */
void jn_ground_nominal_prior(double XR[9], double XT[3]);

/* Host only.  Turn a measured floor (unit normal n_cam from the floor towards the camera, camera height height_m > 0) into XR / XT next to
 * the prior XR0 / XT0:  u0 = XR0^T e_z is the prior's up direction in the camera frame, R_delta the smallest rotation that takes n_cam
 * onto u0 (Rodrigues about n_cam x u0; the identity when they are parallel),  XR = XR0 R_delta,  XT = (XT0.x, XT0.y, height_m).
 * Yaw and XT.x / XT.y stay the prior's.  tilt_deg (may be NULL) receives the angle between n_cam and u0.
 * JN_ERR_INVALID: a NULL pointer, a non-finite or zero normal, height_m <= 0, the normal antiparallel to u0, or a tilt above max_tilt_deg
 * (it found a wall; 30 is a good default).  The outputs are untouched on error, except tilt_deg when the tilt is the reason. */
jn_status jn_ground_align(const double n_cam[3], double height_m, const double XR0[9], const double XT0[3], double max_tilt_deg,
                          double XR[9], double XT[3], double* tilt_deg);

/* Host only.  The joint estimate of several frames: the sums of all planes with status JN_OK are added (exactly the joint fit of those
 * frames' inliers), solved once (jn_ground_solve's arithmetic, Q and crop offsets of sp_prior), and aligned next to sp_prior's XR / XT
 * (jn_ground_align).  JN_ERR_FEW_SUPPORT when no frame is OK or the joint fit is degenerate; JN_ERR_INVALID as jn_ground_align. */
jn_status jn_ground_extrinsics(const jn_ground_plane* planes, int32_t n, const jn_scan_params* sp_prior, double max_tilt_deg,
                               double XR[9], double XT[3], double* tilt_deg);

#ifdef __cplusplus
}
#endif
#endif /* JN_GROUND_H */

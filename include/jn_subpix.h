/* jn_subpix.h — C ABI of the sub-pixel navigation tail of libjn_stereo.so: obstacle scan, costmap and point cloud from FRACTIONAL
 * disparities (ELAS's float D1; the SGM and block-matching modes' int16 maps, integer or 1/16 pixel).
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation rounds its disparity map to mono8 (src/obstacle_avoidance/point_cloud.cpp:422)
 * before anything is reprojected, and jn_stereo.h / jn_costmap.h reproduce that for the reference's own topics: with the shipped rig at
 * 320x180 a point at 3 m has d = 7.3 px, and integer disparities put it at 3.11 m or 2.73 m.  This header defines a SECOND tail next to
 * that one, which reprojects the disparity the matcher computed; the reference-parity tail is unchanged.  Like jn_costmap.h and
 * jn_ground.h it is defined HERE: parity is SELF-REFERENTIAL, its scalar restatement (the checker) lives in the tests
 * (tests/subpix_def.py) — but see "anchor" below, which ties it to entry points whose parity with the reference is established.
 *
 * Definition (all floating-point arithmetic in double, every product, sum, quotient rounded on its own: no contraction).
 *   input          n maps [n][height][width] on the device, in one of
 *                    JN_DISP_F32      float, pixels (ELAS's D1)
 *                    JN_DISP_I16      int16, integer pixels (SGM / block matching)
 *                    JN_DISP_I16_SUB  int16, 1/16 pixel (SGM / block matching with subpixel = 1)
 *                  (the numeric values of jn_ground.h's JN_GROUND_F32 / _I16 / _I16_SUB).
 *   q              every pixel's disparity in 1/16 pixel, int32, exactly as jn_ground.h defines it.  F32: t = rint(16 * d) in float
 *                  (round half to even; 16 * d is exact), q = t; a non-finite d is invalid.  I16: q = 16 * d.  I16_SUB: q = d.
 *   valid          min_q <= q <= 16 * JN_GROUND_MAX_SIDE (F32: the same comparison on t before the conversion).  The matchers' invalid
 *                  values (-10 of ELAS, -1 / -16 of SGM and block matching) are below every admissible min_q.
 *   reprojection   pos = Q [i + crop_offset_x, j + crop_offset_y, q / 16.0, 1]^T (left to right, the constant last; q / 16.0 is exact);
 *                  cam = pos.xyz / pos.w; (X, Y, Z) = XR cam + XT — jn_costmap.h's reprojection with d replaced by q / 16.0.
 *                  Pixels whose homogeneous w is 0 are skipped by the scan and the costmap.
 *   obstacle       a valid pixel with w != 0 whose point is not on the ground model of point_cloud.cpp:166-172, the rule of
 *                  jn_obstacle_scan_cloud:  X < gp_dist_thresh ? Z < gp_height_thresh
 *                                                              : Z < gp_height_thresh + tan(gp_angle_thresh) * (X - gp_dist_thresh)
 *                  (the tangent taken once on the host).  There is no LUT: jn_build_valid_disp_lut is this rule cached per integer d.
 *   scan           dBins [n][sp->bins], dMeta [n][4] by the formulas of jn_obstacle_scan_cloud (:173-184) over the obstacle pixels:
 *                  th = atan2(Y, X), deg = th * 180 / pi_approx, r = sqrt(Y * Y + X * X), bin k = floor(bins * (fov_deg / 2 + -deg) / fov_deg);
 *                  dBins[k] = the smallest r of the bin, JN_SCAN_EMPTY where nothing fell; bins outside [0, bins) are not written;
 *                  dMeta = min th, max th, min r, max r over ALL obstacle pixels (initial values 400, -400, 1e9, -500).
 *                  Minima and maxima of doubles: independent of the order pixels are visited in.
 *   costmap        dHits [n][cells_y][cells_x] u16 saturating at 65535 and dGrid int8: jn_costmap.h's "cell", "hits" and "grid", fed
 *                  with THESE obstacle pixels and THESE bins.  jn_costmap_params.from_cloud is ignored (the rule above is the only
 *                  one; it must still be 0 or 1); every field is validated as jn_obstacle_costmap validates it.
 *   point cloud    float32 xyz triples of every VALID pixel (ground included, as publishPointCloud includes it), in jn_point_cloud's
 *                  i-outer / j-inner order, and their count.  A valid pixel with w = 0 is kept as (0, 0, 0), as jn_point_cloud keeps it.
 *   anchor         on a map whose every q is a multiple of 16 with 2 <= q / 16 <= 255 (and min_q = 32), bins, meta, hits and grid are
 *                  BIT-IDENTICAL to jn_obstacle_scan_cloud / jn_obstacle_costmap(from_cloud = 1) on the u8 map of the same values, and
 *                  the cloud is bit-identical to jn_point_cloud's: the same operations in the same order on the same numbers.
 */
#ifndef JN_SUBPIX_H
#define JN_SUBPIX_H

#include <stdint.h>
#include "jn_stereo.h"
#include "jn_costmap.h"
#include "jn_ground.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum jn_disp_format { JN_DISP_F32 = 0, JN_DISP_I16 = 1, JN_DISP_I16_SUB = 2 } jn_disp_format;   /* == JN_GROUND_F32 / _I16 / _I16_SUB */

typedef struct jn_subpix_params {
  int32_t format;              /* jn_disp_format */
  int32_t min_q;               /* smallest valid disparity in 1/16 pixel, [0, 16 * JN_GROUND_MAX_SIDE] */
} jn_subpix_params;

/* min_q = 32 (d >= 2: the -g route's rule, point_cloud.cpp:326) */
void jn_subpix_params_default(jn_subpix_params* fp, int32_t format);

/* All three calls are synchronous and take device pointers (count: host).  Argument errors — a NULL sp / fp / dDisp / output, n < 1,
 * width or height < 1, an unknown format, min_q outside its range, sp->bins outside [1, 1024], and for the
 * costmap everything jn_obstacle_costmap refuses in cp — return JN_ERR_INVALID before the device is touched; without a device the calls
 * return JN_ERR_NO_DEVICE.
 * jn_subpix_costmap is the scan AND the costmap of the same maps in one pass over the pixels. */
jn_status jn_subpix_scan(int32_t device, const jn_scan_params* sp, const jn_subpix_params* fp, int32_t n, const void* dDisp,
                         int32_t width, int32_t height, double* dBins, double* dMeta);
jn_status jn_subpix_costmap(int32_t device, const jn_scan_params* sp, const jn_costmap_params* cp, const jn_subpix_params* fp, int32_t n,
                            const void* dDisp, int32_t width, int32_t height, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid);
/* one map; dXyz must hold width * height * 3 floats */
jn_status jn_subpix_point_cloud(int32_t device, const jn_scan_params* sp, const jn_subpix_params* fp, const void* dDisp,
                                int32_t width, int32_t height, float* dXyz, int64_t* count);

/* The sub-pixel tail as part of a slot's batch.  From this call on every scan batch submitted on `slot` (jn_elas_submit_scan;
 * jn_sgm_submit_scan with sp != NULL) queues this tail on the slot's stream behind everything the slot already queues (the
 * reference-parity scan, an attached jn_costmap), with the batch's jn_scan_params, the default min_q, and
 *   ELAS   JN_DISP_F32 from the batch's dD1.  A frame that fails (status != 0) leaves dD1 untouched; the tail then scans whatever dD1
 *          held, as the reference-parity tail does;
 *   SGM    JN_DISP_I16, or JN_DISP_I16_SUB for a handle with subpixel = 1, from the batch's dDisp.
 * dBins [max_batch][sp->bins] (room for 1024 bins per frame is always enough), dMeta [max_batch][4]; with cp != NULL also dHits / dGrid
 * [max_batch][cells_y][cells_x].  All are valid after the slot's wait; nothing synchronises with the host in between.  A batch submitted
 * without scan parameters queues nothing extra.  cp == NULL (then dHits and dGrid must be NULL too): the scan only.  cp, dBins, dMeta,
 * dHits, dGrid all NULL: detaches.  Call with no batch in flight on the slot.  A slot with nothing attached queues exactly what it
 * queued before this header existed.
 * With a communicator attached (jn_elas_set_comm) these outputs are the rank's LOCAL ones.  The cross-rig merge is the existing one:
 * bins and meta through jn_scan_allreduce, hits and grid through jn_costmap_allreduce (its grid recomputation is this header's formula).
 * The block matcher (jn_bm.h) has no attach call: call jn_subpix_costmap on the slot's dDisp after jn_bm_wait. */
struct jn_sgm;
jn_status jn_elas_attach_subpix(jn_elas* h, int32_t slot, const jn_costmap_params* cp, double* dBins, double* dMeta, uint16_t* dHits,
                                int8_t* dGrid);
jn_status jn_sgm_attach_subpix(struct jn_sgm* h, int32_t slot, const jn_costmap_params* cp, double* dBins, double* dMeta, uint16_t* dHits,
                               int8_t* dGrid);

#ifdef __cplusplus
}
#endif
#endif /* JN_SUBPIX_H */

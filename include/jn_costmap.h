/* jn_costmap.h — C ABI of the robot-frame obstacle costmap of libjn_stereo.so.
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation hands its navigation stack the 90-bin polar LaserScan
 * (src/obstacle_avoidance/point_cloud.cpp:213-296) and, with -g, a raw point cloud (:298-404); BASELINE.json's north star names a
 * "ground-plane/obstacle-scan costmap" and an "obstacle-grid reduce", which the reference does not contain.
 * This mode is therefore defined HERE: parity is SELF-REFERENTIAL ("parity unpinned" in the sense of SURVEY.md 8c); its scalar
 * restatement (the checker) lives in the tests.  What it produces is the body of a nav_msgs/OccupancyGrid in the robot frame, from the
 * same mono8 disparity map and by the same reprojection the scan uses.
 *
 * Definition (all floating-point arithmetic in double, every product, sum, quotient rounded on its own: no contraction).
 * For one u8 disparity map [height][width] (what jn_disparity_scan / the submit-scan tails write into dDispU8):
 *   obstacle pixels   exactly the pixels the scan bins.  from_cloud = 0: lut0 <= d <= lut1 (point_cloud.cpp:234, the LUT of
 *                     jn_build_valid_disp_lut);  from_cloud = 1: d >= 2 and not on the ground model (:166-172) — the rule of
 *                     jn_obstacle_scan_cloud.  Pixels whose homogeneous w is 0 are skipped, as in the scan.
 *   reprojection      pos = Q [i + crop_offset_x, j + crop_offset_y, d, 1]^T (left to right, the constant last); cam = pos.xyz / pos.w;
 *                     (X, Y, Z) = XR cam + XT (:237-253), as jn_obstacle_scan and jn_point_cloud compute them.
 *   cell              ix = floor((X - origin_x) / resolution), iy = floor((Y - origin_y) / resolution); points with a non-finite
 *                     coordinate or a cell outside [0, cells_x) x [0, cells_y) are dropped.
 *   hits[iy][ix]      number of obstacle pixels in the cell, SATURATING at 65535 (u16; row-major, x along the row:
 *                     nav_msgs/OccupancyGrid's layout).
 *   grid[iy][ix]      int8, the OccupancyGrid convention:
 *                       100  where hits >= min_hits;
 *                         0  (seen free) else, where the cell's centre (xc, yc) = (origin_x + (ix + 0.5) resolution,
 *                            origin_y + (iy + 0.5) resolution) falls, by the scan's own bin formula (:254-263)
 *                            deg = atan2(yc, xc) * 180 / pi_approx,  k = floor(bins * (fov_deg / 2 + -deg) / fov_deg),
 *                            into a bin k in [0, bins) that holds a return (dBins[k] < JN_SCAN_EMPTY - 1) and
 *                            sqrt(yc * yc + xc * xc) + resolution <= dBins[k];
 *                        -1  (unknown) otherwise.  Without bins (dBins = NULL) no cell is free.
 * hits and the 100-cells are integer results, independent of the order pixels are visited in; the free / unknown split depends on one
 * atan2 per cell.
 */
#ifndef JN_COSTMAP_H
#define JN_COSTMAP_H

#include <stdint.h>
#include "jn_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_COSTMAP_MAX_CELLS 512      /* per side */
#define JN_COSTMAP_OCCUPIED 100
#define JN_COSTMAP_FREE 0
#define JN_COSTMAP_UNKNOWN (-1)

typedef struct jn_costmap_params {
  double origin_x, origin_y;   /* robot-frame metres of the corner of cell (0, 0) */
  double resolution;           /* metres per cell, > 0 */
  int32_t cells_x, cells_y;    /* each in [1, JN_COSTMAP_MAX_CELLS] */
  int32_t min_hits;            /* >= 1: obstacle pixels that make a cell occupied */
  int32_t from_cloud;          /* 0: the LUT rule of jn_obstacle_scan, 1: the -g rule of jn_obstacle_scan_cloud */
} jn_costmap_params;

/* origin (0.0, -3.2), resolution 0.05, 128 x 128 cells, min_hits 3, from_cloud 0: the square in front of the robot that the 90-degree
 * scan covers out to 6.4 m */
void jn_costmap_params_default(jn_costmap_params* cp);

/* n maps dDisp [n][height][width] u8 -> dHits [n][cells_y][cells_x] u16, dGrid [n][cells_y][cells_x] int8.  dLut [height][width][2]
 * from jn_build_valid_disp_lut (ignored, may be NULL, with from_cloud = 1); dBins [n][sp->bins] the scan of the same maps, or NULL
 * (no cell is free then).  Synchronous; all device pointers.
 * Argument errors (NULL sp / cp / dDisp / outputs, NULL dLut with from_cloud = 0, n < 1, width or height < 1, sp->bins outside
 * [1, 1024], resolution <= 0 or not finite, cells outside [1, 512], min_hits < 1, from_cloud other than 0 / 1) return JN_ERR_INVALID
 * before the device is touched. */
jn_status jn_obstacle_costmap(int32_t device, const jn_scan_params* sp, const jn_costmap_params* cp, int32_t n, const uint8_t* dDisp,
                              const uint8_t* dLut, int32_t width, int32_t height, const double* dBins, uint16_t* dHits, int8_t* dGrid);

/* The costmap as part of the node's tail.  From this call on every scan batch submitted on `slot` (jn_elas_submit_scan; jn_sgm_submit_scan
 * with sp != NULL) queues the costmap on the slot's stream right behind the scan, from the dDispU8 and dBins that batch wrote (and its
 * dLut), into dHits / dGrid [n][cells_y][cells_x] (room for the handle's max_batch frames); both are valid after the slot's wait.  Nothing
 * synchronises with the host in between.  cp = NULL detaches (dHits / dGrid are ignored and no longer written).  Call with no batch in
 * flight on the slot.  A slot with nothing attached queues exactly what it queued before this header existed.
 * With a communicator attached (jn_elas_set_comm) the grid is built from the batch's LOCAL bins; merge it with jn_costmap_allreduce.
 * The block matcher (jn_bm.h) has no attach call: call jn_obstacle_costmap on the slot's dDispU8 / dBins after jn_bm_wait. */
struct jn_sgm;
jn_status jn_elas_attach_costmap(jn_elas* h, int32_t slot, const jn_costmap_params* cp, uint16_t* dHits, int8_t* dGrid);
jn_status jn_sgm_attach_costmap(struct jn_sgm* h, int32_t slot, const jn_costmap_params* cp, uint16_t* dHits, int8_t* dGrid);

/* Cross-rig merge: afterwards every rank holds dHits = element-wise MAX over the rigs (two rigs seeing one obstacle must not double its
 * count) and dGrid recomputed from the merged hits and dBins (pass the bins jn_scan_allreduce merged; NULL: no cell is free).
 * It travels as the scan's maxima do: ONE ncclAllReduce(ncclMin, ncclDouble) on the communicator's packed buffer, counts negated —
 * 8 bytes per cell on the wire (128 KB per default frame: one latency-bound message).  A rank that feeds the identity (+inf)
 * contributes 0 hits.  Synchronous, bounded by JN_COMM_TIMEOUT_MS like jn_scan_allreduce; every rank must call it with the same n and
 * grid size.  Ordering: NOT concurrently with a handle that has this communicator attached (jn_elas_set_comm) — its workers queue
 * collectives of their own, and all ranks must issue a communicator's collectives in one order. */
jn_status jn_costmap_allreduce(jn_comm* c, const jn_scan_params* sp, const jn_costmap_params* cp, int32_t n, const double* dBins,
                               uint16_t* dHits, int8_t* dGrid);

#ifdef __cplusplus
}
#endif
#endif /* JN_COSTMAP_H */

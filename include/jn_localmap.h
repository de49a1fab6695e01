/* jn_localmap.h — C ABI of the odometry-fused local obstacle map of libjn_stereo.so: a rolling log-odds grid in a FIXED frame, built
 * from disparity maps and the robot's pose, frame after frame.
 *
 * NO REFERENCE COUNTERPART.  Everything sourishg/jackal-navigation publishes is memoryless — the scan, and with this library the costmap
 * (jn_costmap.h) and the sub-pixel tail (jn_subpix.h), are functions of ONE disparity map in the robot frame of that instant.  Its
 * consumer votes over the last 20 whole scans (src/navigation/navigate.cpp:127-149) and forgets what leaves the 90-degree field of view;
 * msg/JackalPose.msg (x, y, theta) is shipped and integrated by nothing.  This mode is the layer a navigation stack puts on top of the
 * per-frame grids: cells are marked where obstacles were seen, cleared where the floor was seen, and remembered when the robot turns
 * away.  Like jn_costmap.h and jn_subpix.h it is defined HERE: parity is SELF-REFERENTIAL, its scalar restatement (the checker) lives in
 * the tests (tests/localmap_def.py) — but see "anchor" below.
 *
 * Definition (all floating-point arithmetic in double, every product, sum, quotient rounded on its own: no contraction).
 *   input          n maps [n][height][width] on the device in one of the three jn_disp_format's, and one jn_pose2d per map: the robot
 *                  (x, y in metres, theta in radians, counter-clockwise) in the fixed ("odom") frame when the map was taken.
 *   q, valid       every pixel's disparity in 1/16 pixel and its validity (with min_q), exactly as jn_subpix.h defines them.
 *   reprojection   robot-frame (X, Y, Z) of a pixel exactly as jn_subpix.h defines it.  Pixels whose homogeneous w is 0 are skipped.
 *   pixel classes  a valid pixel with w != 0 is an OBSTACLE pixel when its point is not on the ground model (jn_subpix.h "obstacle"),
 *                  and a FLOOR pixel otherwise.
 *   world point    c = cos(theta), s = sin(theta), taken once per frame on the host (libm, double);
 *                    Xw = (c * X - s * Y) + x,   Yw = (s * X + c * Y) + y
 *                  (two products, their difference / sum, then one sum, in that order); Z is unchanged.  With the zero pose Xw == X
 *                  and Yw == Y.
 *   window         cells_x x cells_y cells of `resolution` metres, axis-aligned in the fixed frame.  Its cell (0, 0) has the integer
 *                  global index (gx0, gy0) and the corner origin_x = (double)gx0 * resolution, origin_y = (double)gy0 * resolution.
 *                  The cell of a point is jn_costmap.h's "cell" with this origin:
 *                    ix = floor((Xw - origin_x) / resolution), iy = floor((Yw - origin_y) / resolution);
 *                  points with a non-finite Xw, Yw or Z, or a cell outside [0, cells_x) x [0, cells_y), are dropped.  Every array of
 *                  cells is stored [iy][ix], x along the row (nav_msgs/OccupancyGrid's layout).
 *   evidence       per frame f and cell: obst_f = number of obstacle pixels of the frame in the cell, floor_f = number of floor
 *                  pixels, each SATURATING at 65535.  Integers, independent of the order pixels are visited in.
 *   state          L[cell], int16 log-odds in arbitrary units; 0 = nothing known.  The frames of one call are applied IN INDEX ORDER;
 *                  for frame f and every cell
 *                    obst_f  >= min_hits   ->  L = min(L + l_hit, l_max)
 *                    else floor_f >= min_floor  ->  L = max(L - l_miss, l_min)
 *                    else L unchanged.
 *                  One call with n frames therefore equals n calls with one frame each.
 *   grid           int8, the OccupancyGrid convention: 100 where L >= occ_thresh, 0 where L <= free_thresh, -1 otherwise.
 *   recentre       explicit, never implied by an update: gx0 = (int64)floor(x / resolution) - cells_x / 2 (integer division), the same
 *                  for y.  Cells present in both windows keep their L; cells that enter hold 0.  Reset: every L = 0 and the window
 *                  recentred on (0, 0).  A new handle is in the reset state.
 *   anchor         with the zero pose and a window whose origin equals a jn_costmap_params origin (same resolution and size), obst_f is
 *                  BIT-IDENTICAL to jn_subpix_costmap's dHits on the same maps: the same operations in the same order on the same numbers.
 *
 * Why floor sightings clear cells, and not the scan's ray rule.  jn_costmap.h frees a cell only inside a bin that holds a return, so a
 * phantom obstacle (one frame of matcher noise) whose bin is empty in the next frame would never be cleared by it.  "The floor was
 * measured here" is evidence the stereo pipeline actually has, and it is an integer count: no atan2 and no tolerance appear anywhere
 * in this mode, so every output is exact.
 *
 * The suggested thresholds (jn_localmap_params_default) are GUESSES.  Nobody has tuned them on real footage.
 */
#ifndef JN_LOCALMAP_H
#define JN_LOCALMAP_H

#include <stdint.h>
#include "jn_stereo.h"
#include "jn_costmap.h"
#include "jn_subpix.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jn_pose2d { double x, y, theta; } jn_pose2d;   /* the robot in the fixed frame: metres, radians (msg/JackalPose.msg) */

typedef struct jn_localmap_params {
  double resolution;             /* metres per cell, > 0 and finite */
  int32_t cells_x, cells_y;      /* each in [1, JN_COSTMAP_MAX_CELLS] */
  int32_t min_hits;              /* >= 1: obstacle pixels of one frame that count as a hit of the cell */
  int32_t min_floor;             /* >= 1: floor pixels of one frame that count as a miss of the cell */
  int32_t l_hit, l_miss;         /* each in [1, 32767]: what a hit adds, what a miss subtracts */
  int32_t l_min, l_max;          /* -32768 <= l_min < 0 < l_max <= 32767: the clamps */
  int32_t occ_thresh;            /* 0 < occ_thresh <= 32767: L >= occ_thresh is occupied */
  int32_t free_thresh;           /* -32768 <= free_thresh < 0: L <= free_thresh is free */
  int32_t format;                /* jn_disp_format of the maps */
  int32_t min_q;                 /* smallest valid disparity in 1/16 pixel, as in jn_subpix_params */
} jn_localmap_params;

typedef struct jn_localmap jn_localmap;

/* resolution 0.05, 256 x 256 cells, min_hits 3, min_floor 3, l_hit 4, l_miss 1, l_min -8, l_max 16, occ_thresh 4, free_thresh -2,
 * min_q 32: a 12.8 m square; one hit makes an unknown cell occupied, every miss takes one unit back (a cell hit once is below occ_thresh after
 * one miss, a saturated one after thirteen), two misses free an unknown cell.  Untuned guesses (see above). */
void jn_localmap_params_default(jn_localmap_params* p, int32_t format);

/* The handle owns L and the per-call count scratch ([max_batch][2][cells_y][cells_x] u32) on `device`; nothing is allocated per call.
 * max_batch in [1, 256].  A parameter outside its range, a NULL p / out: JN_ERR_INVALID before the device is touched; no device:
 * JN_ERR_NO_DEVICE.  A handle is used by one thread at a time. */
jn_status jn_localmap_create(const jn_localmap_params* p, int32_t max_batch, int32_t device, jn_localmap** out);
void jn_localmap_destroy(jn_localmap* h);

/* every L = 0, window recentred on (0, 0) */
jn_status jn_localmap_reset(jn_localmap* h);
/* the window's centre cell becomes the cell of (x, y).  x, y finite and |x / resolution|, |y / resolution| <= 2^30, else JN_ERR_INVALID */
jn_status jn_localmap_recenter(jn_localmap* h, double x, double y);
/* host only: g0 = (gx0, gy0), origin = (origin_x, origin_y); either may be NULL */
jn_status jn_localmap_window(const jn_localmap* h, int64_t g0[2], double origin[2]);

/* n maps dDisp [n][height][width] (device, the handle's format) with poses[n] (host) -> the evidence of each frame, applied to L in
 * index order.  dObst / dFloor: optional device outputs [n][cells_y][cells_x] u16 (obst_f / floor_f in window order); either may be
 * NULL.  Of sp only Q, the crop offsets, XR / XT and the ground-model fields are read (bins and the field of view are not).
 * Synchronous: everything is queued on one stream in order and waited for.
 * NULL h / sp / poses / dDisp, n outside [1, max_batch], width or height < 1, a non-finite pose, |x / resolution| or |y / resolution|
 * beyond 2^30: JN_ERR_INVALID before the device is touched. */
jn_status jn_localmap_update(jn_localmap* h, const jn_scan_params* sp, int32_t n, const jn_pose2d* poses, const void* dDisp, int32_t width,
                             int32_t height, uint16_t* dObst, uint16_t* dFloor);

/* L -> dLogOdds [cells_y][cells_x] int16 and / or dGrid [cells_y][cells_x] int8 (device, window order); either may be NULL, not both */
jn_status jn_localmap_read(const jn_localmap* h, int16_t* dLogOdds, int8_t* dGrid);

#ifdef __cplusplus
}
#endif
#endif /* JN_LOCALMAP_H */

/* jn_plan.h — C ABI of the local planner of libjn_stereo.so: a CLEARANCE FIELD over an occupancy grid (how far is every cell from the
 * nearest obstacle) and a ROLLOUT OF CANDIDATE ARCS through it toward a waypoint, returning a velocity command (v, omega).
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation decides on one 90-bin scan without memory (src/navigation/navigate.cpp:100-149,
 * this library's jn_nav_vote); its autoNavigateMode (navigate.cpp:282-300, :317) drives to a waypoint ignoring obstacles on the way and
 * says of itself that it does not work yet.  This mode is the step it wanted: it consumes every grid the library makes — the robot-frame
 * grids of jn_obstacle_costmap / jn_subpix_costmap (under the zero pose, with jn_costmap_params' origin) and jn_localmap_read's grid in
 * the fixed frame (with jn_localmap_window's origin).  Like jn_costmap.h and jn_localmap.h it is defined HERE: parity is
 * SELF-REFERENTIAL, its scalar restatement (the checker) lives in the tests (tests/plan_def.py).  The velocity limits are the
 * reference's (navigate.cpp:33-34: 0.6 m/s, 1.3 rad/s — what safeNavigate ramps towards at :326-341); the command is the pair a
 * geometry_msgs/Twist carries there (linear.x, angular.z: navigate.cpp:338-340).  Ramps are the consumer's business.
 *
 * Definition.  Integers wherever possible; all floating-point arithmetic in double, every product, sum, quotient and square root
 * rounded on its own (no contraction); sines and cosines are taken on the host with libm and nowhere else.
 *
 * 1. Clearance field (jn_clearance)
 *   input          n grids [n][cells_y][cells_x] int8 on the device in the OccupancyGrid convention (100 / 0 / -1), stored [iy][ix].
 *   obstacle cell  value 100, or value -1 when unknown_is_obstacle.  Every other value is free.  Cells outside the grid are not
 *                  obstacles.
 *   d2[iy][ix]     u16: the minimum of dx * dx + dy * dy over the obstacle cells (ix + dx, iy + dy) of the same grid with
 *                  dx * dx + dy * dy <= radius * radius; JN_CLEARANCE_FAR (65535) when there is none.  An obstacle cell has 0.
 *                  radius is in cells, 1 <= radius <= JN_CLEARANCE_MAX_RADIUS (255): 255 * 255 = 65025 is what makes it fit 16 bits.
 *                  The squared Euclidean distance in cell units: an integer, independent of the order cells are visited in.
 *
 * 2. Candidates and templates (jn_plan_templates; host)
 *   candidates     K = n_v * n_w, k = iv * n_w + iw:
 *                    v = (v_max * (double)(iv + 1)) / (double)n_v
 *                    w = (w_max * (double)(iw - m)) / (double)m,  m = (n_w - 1) / 2 (n_w is odd: the middle one is exactly 0);
 *                    n_w = 1: w = 0.
 *   template       for step s in [0, steps):  t = (horizon * (double)(s + 1)) / (double)steps;
 *                    w == 0:  (x_t, y_t) = (v * t, 0)
 *                    else     r = v / w,  a = w * t,  (x_t, y_t) = (r * sin(a), r * (1 - cos(a)))
 *                  — the robot-frame point of the arc after t seconds at (v, w), x ahead, y to the left.
 *
 * 3. Evaluation (jn_plan_evaluate; the rollout runs on the device)
 *   frame f        has d2[f] (a clearance field of the handle's grid size), the grid's origin (origin_x, origin_y: the corner of
 *                  cell (0, 0), one per call) and pose[f]; c = cos(theta), s = sin(theta) taken once per frame on the host.
 *   world point    Xw = (c * x_t - s * y_t) + x,  Yw = (s * x_t + c * y_t) + y   (jn_localmap.h's order)
 *   cell           jn_costmap.h's "cell": ix = floor((Xw - origin_x) / resolution), iy = floor((Yw - origin_y) / resolution);
 *                  off the grid when outside [0, cells_x) x [0, cells_y) or not finite; its index is iy * cells_x + ix.
 *   r2             (int)floor(q * q), q = robot_radius / resolution, taken on the host.
 *   record         per candidate, all integers (T = steps):
 *                    t_end     the first step whose cell is off the grid, else T
 *                    t_hit     the first step < t_end with d2 <= r2, else T
 *                    min_d2    the minimum of d2 over the steps before min(t_hit, t_end); JN_CLEARANCE_FAR if there are none
 *                    last_cell the cell index of the last such step; -1 if there are none
 *
 * 4. Choice (jn_plan_choose; host)
 *   admissible     t_hit == T and t_end >= 1 (nothing hit on the part of the arc that is on the grid, and at least one step on it).
 *   score          with (x_t, y_t) the template point of step t_end - 1, (gx, gy) the goal in the frame of the pose:
 *                    ex = (c * x_t - s * y_t) + x,  ey = (s * x_t + c * y_t) + y,  dx = ex - gx,  dy = ey - gy
 *                    dist  = sqrt(dx * dx + dy * dy)
 *                    clear = min(sqrt((double)min_d2) * resolution, clear_cap)
 *                    score = (w_goal * dist - w_clear * clear) - w_speed * v
 *                  candidates are visited in the order of k and one replaces the best so far only with a strictly lower score
 *                  (ties go to the lowest k).
 *   command        the winner's (v, w), its k, status JN_PLAN_OK.  No admissible candidate: (0, 0), candidate -1, status
 *                  JN_PLAN_BLOCKED — never a guess.
 *
 * The defaults (jn_plan_params_default) are GUESSES apart from the two limits.  Nobody has tuned them on real footage.
 */
#ifndef JN_PLAN_H
#define JN_PLAN_H

#include <stdint.h>
#include "jn_stereo.h"
#include "jn_costmap.h"
#include "jn_localmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_CLEARANCE_FAR 65535
#define JN_CLEARANCE_MAX_RADIUS 255
#define JN_PLAN_MAX_BATCH 256
#define JN_PLAN_OK 0
#define JN_PLAN_BLOCKED 1

typedef struct jn_plan_params {
  double v_max;                  /* m/s, > 0 and finite (navigate.cpp:33) */
  double w_max;                  /* rad/s, > 0 and finite (navigate.cpp:34) */
  double horizon;                /* seconds of every arc, > 0 and finite */
  double robot_radius;           /* metres, >= 0, robot_radius / resolution <= 255: a circle around the robot's origin */
  double w_goal;                 /* the chooser's weights and cap, each >= 0 and finite: per metre left to the goal, */
  double w_clear;                /*   per metre of clearance (up to clear_cap), */
  double w_speed;                /*   per m/s */
  double clear_cap;              /* metres */
  int32_t n_v;                   /* [1, 16] */
  int32_t n_w;                   /* odd, [1, 65] */
  int32_t steps;                 /* T, [1, 128] */
  int32_t reserved;              /* 0 */
} jn_plan_params;

typedef struct jn_plan_record { int32_t t_end, t_hit, min_d2, last_cell; } jn_plan_record;
typedef struct jn_plan_cmd { double v, w; int32_t candidate, status; } jn_plan_cmd;

typedef struct jn_plan jn_plan;

/* n grids dGrid [n][cells_y][cells_x] int8 -> dD2 [n][cells_y][cells_x] u16.  Synchronous; both device pointers.
 * NULL dGrid / dD2, n outside [1, JN_PLAN_MAX_BATCH], a side outside [1, JN_COSTMAP_MAX_CELLS], unknown_is_obstacle other than 0 / 1,
 * radius outside [1, JN_CLEARANCE_MAX_RADIUS]: JN_ERR_INVALID before the device is touched. */
jn_status jn_clearance(int32_t device, int32_t n, const int8_t* dGrid, int32_t cells_x, int32_t cells_y, int32_t unknown_is_obstacle,
                       int32_t radius, uint16_t* dD2);

/* v_max 0.6, w_max 1.3 (navigate.cpp:33-34); horizon 2.0 s, robot_radius 0.3 (the Jackal's footprint is about 0.51 x 0.43 m; the
 * reference's clear_side is 0.3), w_goal 1.0, w_clear 0.5, w_speed 0.1, clear_cap 1.0, n_v 3, n_w 11, steps 20.  Untuned guesses (see
 * above). */
void jn_plan_params_default(jn_plan_params* p);

/* Host only, needs no device: the candidates' v [K] and w [K] and their templates xy [K][steps][2] (x_t, y_t); any of the three may be
 * NULL.  Invalid p: JN_ERR_INVALID. */
jn_status jn_plan_templates(const jn_plan_params* p, double* v, double* w, double* xy);

/* The handle owns the templates, the poses and the records [max_batch][K] on `device` (and their pinned host side); nothing is allocated
 * per call.  resolution > 0 and finite, the sides in [1, JN_COSTMAP_MAX_CELLS], max_batch in [1, JN_PLAN_MAX_BATCH].  A parameter
 * outside its range, a NULL p / out: JN_ERR_INVALID before the device is touched; no device: JN_ERR_NO_DEVICE.  One thread at a time. */
jn_status jn_plan_create(const jn_plan_params* p, double resolution, int32_t cells_x, int32_t cells_y, int32_t max_batch, int32_t device,
                         jn_plan** out);
void jn_plan_destroy(jn_plan* h);

/* n fields dD2 [n][cells_y][cells_x] u16 (device), the grids' origin (host, 2 doubles) and poses [n] (host) -> records [n][K] (host).
 * One kernel launch; synchronous.  NULL h / dD2 / origin / poses / records, n outside [1, max_batch], a non-finite origin or pose,
 * |x / resolution| or |y / resolution| of a pose or of the origin beyond 2^30: JN_ERR_INVALID before the device is touched. */
jn_status jn_plan_evaluate(jn_plan* h, int32_t n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses, jn_plan_record* records);

/* Host only, needs no device: the choice among one frame's K records.  goal: 2 doubles in the frame of the pose.  NULL arguments, an
 * invalid p or resolution, a non-finite pose or goal (or one beyond 2^30 cells): JN_ERR_INVALID. */
jn_status jn_plan_choose(const jn_plan_params* p, double resolution, const jn_plan_record* records, const jn_pose2d* pose, const double* goal,
                         jn_plan_cmd* out);

/* jn_plan_evaluate, then jn_plan_choose per frame with goals [n][2] (host) -> cmds [n] (host); records [n][K] (host) may be NULL. */
jn_status jn_plan_command(jn_plan* h, int32_t n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses, const double* goals,
                          jn_plan_cmd* cmds, jn_plan_record* records);

#ifdef __cplusplus
}
#endif
#endif /* JN_PLAN_H */

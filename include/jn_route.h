/* jn_route.h — C ABI of the cost-to-go field of libjn_stereo.so: the least cost of a path through free space from every cell of a
 * clearance field to a goal (a navigation function over the grid), and jn_plan.h's arc rollout scored by that field in place of the
 * straight line to the goal — so that the planner leaves a pocket whose walls the local map remembers.
 *
 * NO REFERENCE COUNTERPART.  sourishg/jackal-navigation's autoNavigateMode (src/navigation/navigate.cpp:282-300) steers at the waypoint
 * ignoring obstacles and says of itself that it does not work; jn_plan.h made the arcs collision-free but still ranks them by
 * sqrt(dx * dx + dy * dy) to the goal, which drives into every dead end between robot and goal and then reports JN_PLAN_BLOCKED from
 * inside it (no candidate turns in place).  Like jn_plan.h this mode is defined HERE: parity is SELF-REFERENTIAL, its scalar restatement
 * (the checker: Dijkstra with a heap) lives in the tests (tests/route_def.py).  jn_plan.h is unchanged; this header adds to it.
 *
 * Definition.  All integers, apart from the goal's cell and the chooser's score, which are double with every operation rounded on its
 * own as in jn_plan.h.
 *
 * 1. Field (jn_route_field)
 *   input          n clearance fields d2 [n][cells_y][cells_x] u16 on the device (jn_clearance), stored [iy][ix]; a goal cell (gx, gy)
 *                  on the grid per field.
 *   passable       a cell with d2 > r2 — the complement of the rollout's hit test d2 <= r2 (jn_plan.h 3), r2 as there,
 *                  0 <= r2 <= 65025.  Cells off the grid are not passable.
 *   moves          from a cell c to its 8 neighbours m = c + (dx, dy), in the FIXED ORDER
 *                    (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,1) (1,-1) (-1,-1);
 *                  step weight w(c, m) = 5 for the four axis moves, 7 for the four diagonal ones.  A diagonal move needs only its target
 *                  to be passable: there is no corner rule, the inflation by r2 already keeps paths off the obstacles.
 *   entering cost  pen(m) = near_penalty when d2[m] <= near_radius * near_radius, else 0.  near_radius in [0, 255] cells, near_penalty
 *                  in [0, 64]; near_radius = 0 adds nothing to what r2 already forbids.
 *   seeds          the passable cells with (ix - gx)^2 + (iy - gy)^2 <= goal_radius^2, goal_radius in [0, 16].  Their number is returned
 *                  per field; 0 means the goal is blocked and that field is JN_ROUTE_UNREACHED everywhere.
 *   g              u16.  Seeds have g = 0.  Every other passable cell c has the minimum over its passable neighbours m of
 *                  w(c, m) + pen(m) + g(m): the least total cost of a path from c to any seed.  A cell that is not passable, has no path,
 *                  or whose minimum is above 65534 has g = JN_ROUTE_UNREACHED (65535).
 *                  Why the cut is well-defined: every step costs at least 5, so every cell on a least-cost path from c has a smaller
 *                  value than c, and a cell whose true value is at most 65534 gets exactly that value whatever was cut above it.  Sums are
 *                  formed in 32 bits and those above 65534 dropped.
 *                  The result does not depend on the order cells are relaxed in: any schedule that relaxes to a fixed point gives it.
 *   in metres      g * resolution / 5 is the length of the path when no penalty applies, in the 5-7 chamfer metric.  Between two cells
 *                  a and b cells apart (a >= b >= 0) with nothing in the way g = 5 a + 2 b, so g / 5 = a + 0.4 b against
 *                  sqrt(a * a + b * b): with tan(t) = b / a the ratio is cos(t) + 0.4 sin(t) on [0, 45 degrees], whose maximum is
 *                  sqrt(1.16) = 1.0770 at tan(t) = 0.4 and whose minimum is 1.4 / sqrt(2) = 0.98995 at 45 degrees.  So the figure is
 *                  between 1.01 % short and 7.70 % long of the straight line, and the same per straight piece of a path round obstacles.
 *                  Every penalised cell entered adds near_penalty / 5 cells on top.
 *   radius         the clearance field says JN_CLEARANCE_FAR beyond the radius it was made with.  A field made with a radius below
 *                  max(ceil(sqrt(r2)), near_radius) would turn cells that should hit or be penalised into free ones without a word; the
 *                  caller of jn_clearance owns that radius, and the Python wrapper refuses a smaller one where it makes the field itself.
 *
 * 2. Goal cell (jn_route_goal_cell; host)
 *   ix = floor((X - origin_x) / resolution), iy likewise — jn_costmap.h's "cell" arithmetic — then each clamped to [0, cells - 1]: a goal
 *   beyond the map lands on the nearest border cell.  A non-finite goal is JN_ERR_INVALID.
 *
 * 3. Evaluation (jn_route_evaluate; rollout and gather run on the device)
 *   jn_plan_evaluate's records, bit for bit, and togo [n][K] u16: g at the record's last_cell, JN_ROUTE_UNREACHED when last_cell == -1.
 *
 * 4. Choice (jn_route_choose; host) — jn_plan.h 4 with two changes:
 *   admissible     t_hit == T, t_end >= 1 and togo != JN_ROUTE_UNREACHED
 *   dist           = ((double)togo * resolution) / 5.0
 *   clear, score, the order of visits, the tie rule and the result are jn_plan.h's; no admissible candidate: (0, 0), candidate -1,
 *   JN_PLAN_BLOCKED.
 *
 * 5. Path (jn_route_trace; host) on a host copy of one field's g and d2 with the same r2 and parameters, from a start cell:
 *   while g(c) != 0 step to the first neighbour m in the fixed order with w(c, m) + pen(m) + g(m) == g(c).  g falls at every step, so
 *   the walk ends.  A start off the grid or with g == JN_ROUTE_UNREACHED: length 0, JN_ROUTE_NO_ROUTE.
 *
 * The defaults (jn_route_params_default) are GUESSES.  Nobody has tuned them on real footage.
 */
#ifndef JN_ROUTE_H
#define JN_ROUTE_H

#include <stdint.h>
#include "jn_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JN_ROUTE_UNREACHED 65535
#define JN_ROUTE_MAX_R2 65025
#define JN_ROUTE_MAX_NEAR_RADIUS 255
#define JN_ROUTE_MAX_NEAR_PENALTY 64
#define JN_ROUTE_MAX_GOAL_RADIUS 16
#define JN_ROUTE_OK 0
#define JN_ROUTE_NO_ROUTE 1
/* jn_route_stats.form: which kernel form made the field */
#define JN_ROUTE_FORM_WHOLE 0
#define JN_ROUTE_FORM_TILED 1

typedef struct jn_route_params {
  int32_t near_radius;           /* cells, [0, 255] */
  int32_t near_penalty;          /* cost units (5 per cell), [0, 64] */
  int32_t goal_radius;           /* cells, [0, 16] */
  int32_t reserved;              /* 0 */
} jn_route_params;

/* How a field was made.  rounds: relaxation rounds (four sweeps each) of the busiest workgroup, summed over the launches. */
typedef struct jn_route_stats { int32_t form, launches, rounds, reserved; } jn_route_stats;

/* near_radius 10, near_penalty 3, goal_radius 2.  Untuned guesses (see above). */
void jn_route_params_default(jn_route_params* rp);

/* Host only, needs no device.  origin, goal: 2 doubles each; cell: 2 int32 (ix, iy).  NULL arguments, a resolution that is not positive
 * and finite, a side outside [1, JN_COSTMAP_MAX_CELLS], a non-finite origin or goal: JN_ERR_INVALID. */
jn_status jn_route_goal_cell(double resolution, int32_t cells_x, int32_t cells_y, const double* origin, const double* goal, int32_t* cell);

/* n fields dD2 [n][cells_y][cells_x] u16 (device) and goal cells [n][2] (host; ix, iy) -> dTogo [n][cells_y][cells_x] u16 (device) and
 * seeds [n] (host).  stats may be NULL.  Synchronous.  Exact at every size; the launches of the tiled form are bounded by what the
 * definition allows (one cell settled per launch) and passing the bound is JN_ERR_INTERNAL, never an unfinished field.
 * NULL dD2 / goal_cells / dTogo / seeds / rp, n outside [1, JN_PLAN_MAX_BATCH], a side outside [1, JN_COSTMAP_MAX_CELLS], r2 outside
 * [0, JN_ROUTE_MAX_R2], a parameter outside its range, a goal cell off the grid: JN_ERR_INVALID before the device is touched. */
jn_status jn_route_field(int32_t device, int32_t n, const uint16_t* dD2, int32_t cells_x, int32_t cells_y, int32_t r2,
                         const jn_route_params* rp, const int32_t* goal_cells, uint16_t* dTogo, int32_t* seeds, jn_route_stats* stats);

/* jn_plan_evaluate with the fields dTogo [n][cells_y][cells_x] u16 (device) next to dD2 -> records [n][K] and togo [n][K] u16 (host).
 * Two kernel launches; synchronous.  jn_plan_evaluate's conditions, and NULL dTogo / togo: JN_ERR_INVALID before the device is touched. */
jn_status jn_route_evaluate(jn_plan* h, int32_t n, const uint16_t* dD2, const uint16_t* dTogo, const double* origin, const jn_pose2d* poses,
                            jn_plan_record* records, uint16_t* togo);

/* Host only, needs no device: the choice among one frame's K records and togo values.  NULL arguments, an invalid p or resolution:
 * JN_ERR_INVALID. */
jn_status jn_route_choose(const jn_plan_params* p, double resolution, const jn_plan_record* records, const uint16_t* togo, jn_plan_cmd* out);

/* jn_route_evaluate, then jn_route_choose per frame -> cmds [n] (host); records [n][K] and togo [n][K] (host) may be NULL. */
jn_status jn_route_command(jn_plan* h, int32_t n, const uint16_t* dD2, const uint16_t* dTogo, const double* origin, const jn_pose2d* poses,
                           jn_plan_cmd* cmds, jn_plan_record* records, uint16_t* togo);

/* Host only, needs no device: the path from (start_x, start_y) over host copies g and d2 [cells_y][cells_x] -> cells [*length] (indices
 * iy * cells_x + ix, the start first, a seed last) and *status (JN_ROUTE_OK / JN_ROUTE_NO_ROUTE).  NULL arguments, a side, r2 or
 * parameter outside its range, capacity < 0: JN_ERR_INVALID.  A path longer than `capacity`, or a g that is not the field of these
 * inputs (no neighbour continues the path): JN_ERR_INVALID with *length = 0 — never a cut path. */
jn_status jn_route_trace(const uint16_t* g, const uint16_t* d2, int32_t cells_x, int32_t cells_y, int32_t r2, const jn_route_params* rp,
                         int32_t start_x, int32_t start_y, int32_t* cells, int32_t capacity, int32_t* length, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* JN_ROUTE_H */

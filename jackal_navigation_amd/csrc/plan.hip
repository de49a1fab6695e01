// plan.hip — the local planner (include/jn_plan.h): the clearance field of an occupancy grid (the exact squared Euclidean distance to
// the nearest obstacle cell, cut at a radius) and the rollout of candidate arcs through it.  Its kernels, the handle and the C entry
// points.  Product code.
//
// No reference counterpart; the definition is in jn_plan.h, its scalar restatement (the checker) in tests/plan_def.py.  The cell of a
// point is nav_tail.h's nav_cell, the one costmap.hip, subpix.hip and localmap.hip call.
//
// Two kernels.
//   k_clearance     one launch, one form for every grid size and radius.  The transform separates: g(y, x) = the distance from (x, y) to
//                   the nearest obstacle in its own COLUMN, then d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2.  A workgroup owns a
//                   band of kClrBand rows (batches on blockIdx.z) and stages the band plus `radius` rows of halo above and below as
//                   obstacle BITS, one column per 32-bit word lane ([word][x], x fastest): 17 words x 512 columns = 34 KB at the largest
//                   radius, so the halo never outgrows the LDS and there is no second form.  The column pass is a find-first-set /
//                   count-leading-zeros walk over at most 9 words up and 9 down; g^2 goes to a u16 plane [band row][x] in LDS (g <= 255,
//                   so g^2 fits).  The row pass has lanes on consecutive x: every LDS read of the loop is consecutive across the wave, a
//                   lane stops taking part as soon as dx^2 alone reaches its running minimum, the wave leaves when all its lanes have.
//   k_plan_rollout  one thread per (candidate, frame): the template points through the frame's pose into cells, the first step off the
//                   grid, the first hit, the minimum on the way.  Templates are stored [step][candidate] so a wave's loads are
//                   consecutive.  No transcendental: sines and cosines are the host's.
// The choice among the records is host code (jn_plan_choose): K candidates, a dozen double operations each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "nav_tail.h"
#include "plan_handle.h"

namespace jnav {
namespace {

constexpr int kFar = JN_CLEARANCE_FAR;
constexpr int kClrBand = 8;                                                             // rows of d2 per workgroup
constexpr int kClrThreads = 512;
constexpr int kClrMaxWords = (kClrBand + 2 * JN_CLEARANCE_MAX_RADIUS + 31) / 32;        // 17: band + halo, in 32-row words

// grid [n][cy][cx] int8 -> d2 [n][cy][cx] u16.  gridDim = (ceil(cy / kClrBand), 1, n).  Bit i of a column's word w is row
// y0 - R + 32 w + i; rows outside the grid are 0 bits (not obstacles).
__global__ void __launch_bounds__(kClrThreads) k_clearance(const int8_t* __restrict__ grid, int cx, int cy, int unk, int R, uint16_t* __restrict__ d2) {
  __shared__ uint32_t bits[kClrMaxWords * JN_COSTMAP_MAX_CELLS];
  __shared__ uint16_t g2[kClrBand * JN_COSTMAP_MAX_CELLS];
  const int frame = blockIdx.z, y0 = blockIdx.x * kClrBand;
  const int base = y0 - R;
  const int nw = (kClrBand + 2 * R + 31) >> 5;                                          // <= kClrMaxWords
  const int8_t* __restrict__ g = grid + (size_t)frame * cx * cy;

  // the band and its halo as bits: 32 rows of one column per task, lanes on consecutive columns (every load a coalesced row piece)
  for (int t = threadIdx.x; t < nw * cx; t += kClrThreads) {
    const int w = t / cx, x = t - w * cx;
    const int r0 = base + 32 * w;
    uint32_t m = 0;
    if (r0 + 31 >= 0 && r0 < cy) {
      int8_t v[32];
#pragma unroll
      for (int b = 0; b < 32; b++) {
        const int r = r0 + b;
        v[b] = (r >= 0 && r < cy) ? g[(size_t)r * cx + x] : (int8_t)0;
      }
#pragma unroll
      for (int b = 0; b < 32; b++) m |= (uint32_t)(v[b] == 100 || (unk && v[b] == -1)) << b;
    }
    bits[t] = m;
  }
  __syncthreads();

  // column pass: the nearest set bit above and below the row's own bit p, at most R away
  for (int t = threadIdx.x; t < kClrBand * cx; t += kClrThreads) {
    const int yb = t / cx, x = t - yb * cx;
    const int p = R + yb;
    int best = R + 1;
    {
      int w = p >> 5;
      uint32_t m = bits[w * cx + x] & (~0u << (p & 31));
      for (;;) {
        if (m) { best = min(best, (w << 5) + __ffs((int)m) - 1 - p); break; }
        if (++w >= nw || (w << 5) - p > R) break;
        m = bits[w * cx + x];
      }
    }
    {
      int w = p >> 5;
      uint32_t m = bits[w * cx + x] & (~0u >> (31 - (p & 31)));
      for (;;) {
        if (m) { best = min(best, p - ((w << 5) + 31 - __clz((int)m))); break; }
        if (--w < 0 || p - ((w << 5) + 31) > R) break;
        m = bits[w * cx + x];
      }
    }
    g2[t] = (uint16_t)(best <= R ? best * best : kFar);
  }
  __syncthreads();

  // row pass: lanes on consecutive x.  `best` starts at R^2 + 1 ("nothing within R"), so dx stops at R + 1 at the latest.
  const int R2 = R * R;
  for (int t0 = 0; t0 < kClrBand * cx; t0 += kClrThreads) {
    const int t = t0 + threadIdx.x;
    const bool on = t < kClrBand * cx;
    const int yb = on ? t / cx : 0, x = on ? t - yb * cx : 0;
    const bool live = on && y0 + yb < cy;
    const uint16_t* row = g2 + yb * cx;
    int best = live ? min((int)row[x], R2 + 1) : 0;
    for (int dx = 1;; dx++) {
      const int dd = dx * dx;
      if (__all(dd >= best)) break;                                                     // wave-uniform
      if (dd < best) {
        if (x - dx >= 0) best = min(best, dd + (int)row[x - dx]);
        if (x + dx < cx) best = min(best, dd + (int)row[x + dx]);
      }
    }
    if (live) d2[((size_t)frame * cy + (y0 + yb)) * cx + x] = (uint16_t)(best <= R2 ? best : kFar);
  }
}

struct PlDev {
  NavGrid c;
  int K, T, r2;
};

// tpl [T][K] (x_t, y_t); d2 [n][cells]; rec [n][K].  gridDim = (ceil(K / 256), n).
__global__ void __launch_bounds__(256) k_plan_rollout(PlDev s, const PlPose* __restrict__ poses, const double2* __restrict__ tpl,
                                                      const uint16_t* __restrict__ d2, jn_plan_record* __restrict__ rec) {
  const int k = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
  if (k >= s.K) return;
  const PlPose p = poses[frame];
  const uint16_t* __restrict__ field = d2 + (size_t)frame * s.c.cx * s.c.cy;
  const double z = 0.0;
  int t_end = s.T, t_hit = s.T, mn = kFar, last = -1;
  for (int st = 0; st < s.T; st++) {
    const double2 q = tpl[(size_t)st * s.K + k];
    const double Xw = __dadd_rn(__dsub_rn(__dmul_rn(p.c, q.x), __dmul_rn(p.s, q.y)), p.x);
    const double Yw = __dadd_rn(__dadd_rn(__dmul_rn(p.s, q.x), __dmul_rn(p.c, q.y)), p.y);
    const int cell = nav_cell(s.c, Xw, Yw, z);
    if (cell < 0) { t_end = st; break; }
    const int d = field[cell];
    if (d <= s.r2) { t_hit = st; break; }
    mn = min(mn, d);
    last = cell;
  }
  rec[(size_t)frame * s.K + k] = jn_plan_record{t_end, t_hit, mn, last};
}

// jn_plan.h "choice" of one frame; c / s: the pose's cosine and sine
void pl_choose(const jn_plan_params& p, double res, const jn_plan_record* rec, double c, double s, double x, double y, const double* goal,
               jn_plan_cmd* out) {
  const int K = p.n_v * p.n_w, T = p.steps;
  double best = 0.;
  *out = jn_plan_cmd{0., 0., -1, JN_PLAN_BLOCKED};
  for (int k = 0; k < K; k++) {
    const jn_plan_record& r = rec[k];
    if (r.t_hit != T || r.t_end < 1 || r.t_end > T) continue;
    double v, w, xt, yt;
    pl_candidate(p, k, v, w);
    pl_point(p, v, w, r.t_end - 1, xt, yt);
    const double ex = (c * xt - s * yt) + x, ey = (s * xt + c * yt) + y;
    const double dx = ex - goal[0], dy = ey - goal[1];
    const double dist = std::sqrt(dx * dx + dy * dy);
    const double clear = std::min(std::sqrt((double)r.min_d2) * res, p.clear_cap);
    const double score = (p.w_goal * dist - p.w_clear * clear) - p.w_speed * v;
    if (out->candidate < 0 || score < best) {
      best = score;
      *out = jn_plan_cmd{v, w, k, JN_PLAN_OK};
    }
  }
}

}  // namespace

// plan_handle.h: the arguments of evaluate / command that do not depend on the output
bool pl_call_valid(const jn_plan* h, int n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses) {
  if (!h || !dD2 || !origin || !poses || n < 1 || n > h->max_batch) return false;
  if (!pl_coord_valid(origin[0], h->res) || !pl_coord_valid(origin[1], h->res)) return false;
  for (int f = 0; f < n; f++)
    if (!pl_pose_valid(poses[f], h->res)) return false;
  return true;
}

// plan_handle.h: the rollout of n frames on the null stream, the records on their way into h->h_rec
jn_status pl_enqueue(jn_plan* h, int n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses) {
  for (int f = 0; f < n; f++) h->h_poses[f] = PlPose{std::cos(poses[f].theta), std::sin(poses[f].theta), poses[f].x, poses[f].y};
  HIP_TRY(hipSetDevice(h->device));
  PlDev s;
  s.c = NavGrid{origin[0], origin[1], h->res, h->cx, h->cy};
  s.K = h->K; s.T = h->p.steps; s.r2 = h->r2;
  HIP_TRY(hipMemcpyAsync(h->d_poses, h->h_poses, sizeof(PlPose) * (size_t)n, hipMemcpyHostToDevice, nullptr));
  hipLaunchKernelGGL(k_plan_rollout, dim3((unsigned)((h->K + 255) / 256), (unsigned)n), dim3(256), 0, nullptr, s, h->d_poses, h->d_tpl, dD2, h->d_rec);
  HIP_TRY(hipMemcpyAsync(h->h_rec, h->d_rec, sizeof(jn_plan_record) * (size_t)n * h->K, hipMemcpyDeviceToHost, nullptr));
  return JN_OK;
}

}  // namespace jnav

using namespace jnav;

namespace {

void pl_free(jn_plan* h) {
  h->own.release();
  delete h;
}

// the rollout of n frames into h->h_rec; the poses' cosines and sines stay in h->h_poses
jn_status pl_evaluate(jn_plan* h, int n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses) {
  const jn_status e = pl_enqueue(h, n, dD2, origin, poses);
  if (e != JN_OK) return e;
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // namespace

extern "C" {

jn_status jn_clearance(int32_t device, int32_t n, const int8_t* dGrid, int32_t cells_x, int32_t cells_y, int32_t unknown_is_obstacle,
                       int32_t radius, uint16_t* dD2) {
  if (!dGrid || !dD2 || n < 1 || n > JN_PLAN_MAX_BATCH || cells_x < 1 || cells_x > JN_COSTMAP_MAX_CELLS || cells_y < 1 ||
      cells_y > JN_COSTMAP_MAX_CELLS || (unknown_is_obstacle != 0 && unknown_is_obstacle != 1) || radius < 1 || radius > JN_CLEARANCE_MAX_RADIUS)
    return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_clearance, dim3((unsigned)((cells_y + kClrBand - 1) / kClrBand), 1, (unsigned)n), dim3(kClrThreads), 0, nullptr, dGrid, cells_x,
                     cells_y, unknown_is_obstacle, radius, dD2);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

void jn_plan_params_default(jn_plan_params* p) {
  p->v_max = 0.6; p->w_max = 1.3;                                     // navigate.cpp:33-34
  p->horizon = 2.0; p->robot_radius = 0.3;                            // untuned guesses from here on (jn_plan.h)
  p->w_goal = 1.0; p->w_clear = 0.5; p->w_speed = 0.1; p->clear_cap = 1.0;
  p->n_v = 3; p->n_w = 11; p->steps = 20; p->reserved = 0;
}

jn_status jn_plan_templates(const jn_plan_params* p, double* v, double* w, double* xy) {
  if (!pl_params_valid(p)) return JN_ERR_INVALID;
  const int K = p->n_v * p->n_w;
  for (int k = 0; k < K; k++) {
    double vk, wk;
    pl_candidate(*p, k, vk, wk);
    if (v) v[k] = vk;
    if (w) w[k] = wk;
    if (xy)
      for (int s = 0; s < p->steps; s++) pl_point(*p, vk, wk, s, xy[((size_t)k * p->steps + s) * 2], xy[((size_t)k * p->steps + s) * 2 + 1]);
  }
  return JN_OK;
}

jn_status jn_plan_create(const jn_plan_params* p, double resolution, int32_t cells_x, int32_t cells_y, int32_t max_batch, int32_t device,
                         jn_plan** out) {
  if (out) *out = nullptr;
  if (!pl_params_valid(p) || !out || !pl_resolution_valid(p, resolution) || cells_x < 1 || cells_x > JN_COSTMAP_MAX_CELLS || cells_y < 1 ||
      cells_y > JN_COSTMAP_MAX_CELLS || max_batch < 1 || max_batch > JN_PLAN_MAX_BATCH)
    return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  jn_plan* h = new (std::nothrow) jn_plan();
  if (!h) return JN_ERR_INTERNAL;
  h->p = *p; h->res = resolution; h->cx = cells_x; h->cy = cells_y; h->device = device; h->max_batch = max_batch;
  h->K = p->n_v * p->n_w;
  const double q = p->robot_radius / resolution;
  h->r2 = (int)std::floor(q * q);
  const int T = p->steps;
  std::vector<double2> tpl((size_t)T * h->K);
  for (int k = 0; k < h->K; k++) {
    double v, w;
    pl_candidate(*p, k, v, w);
    for (int s = 0; s < T; s++) pl_point(*p, v, w, s, tpl[(size_t)s * h->K + k].x, tpl[(size_t)s * h->K + k].y);
  }
  if (h->own.alloc(&h->d_tpl, tpl.size()) != hipSuccess || h->own.alloc(&h->d_poses, (size_t)max_batch) != hipSuccess ||
      h->own.pinned(&h->h_poses, (size_t)max_batch) != hipSuccess || h->own.alloc(&h->d_rec, (size_t)max_batch * h->K) != hipSuccess ||
      h->own.pinned(&h->h_rec, (size_t)max_batch * h->K) != hipSuccess ||
      hipMemcpy(h->d_tpl, tpl.data(), sizeof(double2) * tpl.size(), hipMemcpyHostToDevice) != hipSuccess) {
    pl_free(h);
    return JN_ERR_NO_DEVICE;
  }
  *out = h;
  return JN_OK;
}

void jn_plan_destroy(jn_plan* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  pl_free(h);
}

jn_status jn_plan_evaluate(jn_plan* h, int32_t n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses, jn_plan_record* records) {
  if (!pl_call_valid(h, n, dD2, origin, poses) || !records) return JN_ERR_INVALID;
  const jn_status e = pl_evaluate(h, n, dD2, origin, poses);
  if (e != JN_OK) return e;
  memcpy(records, h->h_rec, sizeof(jn_plan_record) * (size_t)n * h->K);
  return JN_OK;
}

jn_status jn_plan_choose(const jn_plan_params* p, double resolution, const jn_plan_record* records, const jn_pose2d* pose, const double* goal,
                         jn_plan_cmd* out) {
  if (!pl_params_valid(p) || !pl_resolution_valid(p, resolution) || !records || !pose || !goal || !out || !pl_pose_valid(*pose, resolution) ||
      !pl_coord_valid(goal[0], resolution) || !pl_coord_valid(goal[1], resolution))
    return JN_ERR_INVALID;
  pl_choose(*p, resolution, records, std::cos(pose->theta), std::sin(pose->theta), pose->x, pose->y, goal, out);
  return JN_OK;
}

jn_status jn_plan_command(jn_plan* h, int32_t n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses, const double* goals,
                          jn_plan_cmd* cmds, jn_plan_record* records) {
  if (!pl_call_valid(h, n, dD2, origin, poses) || !goals || !cmds) return JN_ERR_INVALID;
  for (int f = 0; f < n; f++)
    if (!pl_coord_valid(goals[2 * f], h->res) || !pl_coord_valid(goals[2 * f + 1], h->res)) return JN_ERR_INVALID;
  const jn_status e = pl_evaluate(h, n, dD2, origin, poses);
  if (e != JN_OK) return e;
  for (int f = 0; f < n; f++) {
    const PlPose& q = h->h_poses[f];
    pl_choose(h->p, h->res, h->h_rec + (size_t)f * h->K, q.c, q.s, q.x, q.y, goals + 2 * f, cmds + f);
  }
  if (records) memcpy(records, h->h_rec, sizeof(jn_plan_record) * (size_t)n * h->K);
  return JN_OK;
}

}  // extern "C"

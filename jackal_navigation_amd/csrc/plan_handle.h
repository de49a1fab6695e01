// plan_handle.h — the jn_plan handle and the host pieces of the planner's definition (include/jn_plan.h) that plan.hip and route.hip both
// use: argument checks, the candidates and their templates, and the rollout of a batch enqueued on the null stream.  Product code.
//
// plan.hip defines what is declared here without a body and keeps the kernels; route.hip (include/jn_route.h) scores the same records by
// its cost-to-go field and keeps its per-handle buffers in the fields at the end of the handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "dev_owner.h"
#include "hip_try.h"
#include "../../include/jn_plan.h"

namespace jnav {

constexpr double kPlMaxIndex = 1073741824.0;      // 2^30, as jn_localmap.h

struct PlPose { double c, s, x, y; };             // cos / sin of theta taken on the host

inline bool pl_pos(double v) { return std::isfinite(v) && v > 0.; }
inline bool pl_nonneg(double v) { return std::isfinite(v) && v >= 0.; }

inline bool pl_params_valid(const jn_plan_params* p) {
  return p && pl_pos(p->v_max) && pl_pos(p->w_max) && pl_pos(p->horizon) && pl_nonneg(p->robot_radius) && pl_nonneg(p->w_goal) &&
         pl_nonneg(p->w_clear) && pl_nonneg(p->w_speed) && pl_nonneg(p->clear_cap) && p->n_v >= 1 && p->n_v <= 16 && p->n_w >= 1 && p->n_w <= 65 &&
         (p->n_w & 1) && p->steps >= 1 && p->steps <= 128 && p->reserved == 0;
}
// the resolution, and the robot's radius in cells (r2 must stay below the "far" value)
inline bool pl_resolution_valid(const jn_plan_params* p, double res) { return pl_pos(res) && p->robot_radius / res <= (double)JN_CLEARANCE_MAX_RADIUS; }
inline bool pl_coord_valid(double v, double res) { return std::isfinite(v) && std::fabs(v / res) <= kPlMaxIndex; }
inline bool pl_pose_valid(const jn_pose2d& q, double res) { return pl_coord_valid(q.x, res) && pl_coord_valid(q.y, res) && std::isfinite(q.theta); }

// jn_plan.h "candidates" and "template": every operation on its own
inline void pl_candidate(const jn_plan_params& p, int k, double& v, double& w) {
  const int iv = k / p.n_w, iw = k - iv * p.n_w, m = (p.n_w - 1) / 2;
  v = (p.v_max * (double)(iv + 1)) / (double)p.n_v;
  w = m == 0 ? 0. : (p.w_max * (double)(iw - m)) / (double)m;
}
inline void pl_point(const jn_plan_params& p, double v, double w, int s, double& x, double& y) {
  const double t = (p.horizon * (double)(s + 1)) / (double)p.steps;
  if (w == 0.) { x = v * t; y = 0.; return; }
  const double r = v / w, a = w * t;
  x = r * std::sin(a);
  y = r * (1. - std::cos(a));
}

}  // namespace jnav

struct jn_plan {
  jn_plan_params p;
  double res = 0.;
  int cx = 0, cy = 0, K = 0, r2 = 0, device = 0, max_batch = 0;
  jnav::DevOwner own;
  double2* d_tpl = nullptr;            // [steps][K]
  jnav::PlPose* d_poses = nullptr;     // [max_batch]
  jnav::PlPose* h_poses = nullptr;     // pinned
  jn_plan_record* d_rec = nullptr;     // [max_batch][K]
  jn_plan_record* h_rec = nullptr;     // pinned
  uint16_t* d_togo = nullptr;          // [max_batch][K]: route.hip's, made at its first call on the handle
  uint16_t* h_togo = nullptr;          // pinned
};

namespace jnav {

// the arguments of evaluate / command that do not depend on the output
__attribute__((visibility("hidden"))) bool pl_call_valid(const jn_plan* h, int n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses);

// The rollout of n frames on the null stream: poses up, the kernel, the records down into h->h_rec.  Nothing is waited for; the poses'
// cosines and sines stay in h->h_poses.  Sets the handle's device.
__attribute__((visibility("hidden"))) jn_status pl_enqueue(jn_plan* h, int n, const uint16_t* dD2, const double* origin, const jn_pose2d* poses);

}  // namespace jnav

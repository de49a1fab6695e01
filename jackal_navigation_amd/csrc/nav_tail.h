// nav_tail.h — what the scan and the navigation tails behind the matchers share (scan.hip, costmap.hip, subpix.hip, ground.hip,
// localmap.hip, postfilter.hip; the slots of elas_handle.h and sgm.hip).  Product code.
//
// Host side: the calling thread's device scratch, and NavTails — the tails attached to one slot of a handle.
// Device side (.hip files only): the reprojection and the ground model, cell and bin of a point, the order-preserving double <-> uint64
// map, the wave-combined add, and the conversion of a map element to 1/16 pixel.  Every double operation is individually rounded on
// purpose (include/jn_costmap.h, jn_subpix.h: the bar is bit-identity); do not contract or reassociate an expression here.
// The scan itself (scan.hip) is built on the same definitions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "hip_try.h"
#include "kernels.h"

namespace jnav {

// Grow-only scratch of the synchronous entry points, one buffer per calling thread (on the device it was last asked for): no hipMalloc /
// hipFree (a device-wide sync) per call.  Every caller synchronises before it returns, so the buffer is free again at the next call.
inline hipError_t thread_scratch(int device, size_t bytes, void** out) {
  struct Scratch { void* p = nullptr; size_t cap = 0; int dev = -1; };
  static thread_local Scratch sc;
  if (sc.dev != device || sc.cap < bytes) {
    if (sc.p) { (void)hipSetDevice(sc.dev); (void)hipFree(sc.p); (void)hipSetDevice(device); sc.p = nullptr; sc.cap = 0; }
    const hipError_t e = hipMalloc(&sc.p, bytes);
    if (e != hipSuccess) return e;
    sc.cap = bytes; sc.dev = device;
  }
  *out = sc.p;
  return hipSuccess;
}

// The tails attached to one slot of an ELAS or SGM handle (jn_*_attach_costmap, include/jn_costmap.h; jn_*_attach_subpix,
// include/jn_subpix.h; jn_sgm_attach_postfilter, include/jn_postfilter.h) and their device scratch.  A plain value: a copy refers to the same scratch, release() frees it.  The handle
// calls attach_* only while the slot is idle, so nothing reads the scratch a call replaces.
struct NavTails {
  struct Costmap { bool on = false; jn_costmap_params cp = {}; uint16_t* hits = nullptr; int8_t* grid = nullptr; };
  struct Subpix { bool on = false, has_cp = false; jn_costmap_params cp = {}; double* bins = nullptr; double* meta = nullptr; uint16_t* hits = nullptr; int8_t* grid = nullptr; };
  Costmap cm; void* cm_acc = nullptr; size_t cm_acc_bytes = 0;   // the accumulation grid [max_batch][cells] u32
  Subpix sx; void* sx_scratch = nullptr; size_t sx_bytes = 0;    // subpix_scratch_bytes(cp, max_batch)
  struct Postfilter { bool on = false; jn_postfilter_params fp = {}; uint32_t* stats = nullptr; };
  Postfilter pf; void* pf_scratch = nullptr; size_t pf_bytes = 0; // postfilter_scratch_bytes(fp, max_batch, W, H, in place)

  static jn_status grow(int device, size_t need, void** p, size_t* cap) {
    if (need <= *cap) return JN_OK;
    HIP_TRY(hipSetDevice(device));
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    HIP_TRY(hipMalloc(p, need));
    *cap = need;
    return JN_OK;
  }

  // cp == nullptr detaches
  jn_status attach_costmap(int device, int max_batch, const jn_costmap_params* cp, uint16_t* dHits, int8_t* dGrid) {
    if (cp && (!costmap_params_valid(cp) || !dHits || !dGrid)) return JN_ERR_INVALID;
    if (!cp) { cm = Costmap(); return JN_OK; }
    const jn_status e = grow(device, costmap_scratch_bytes(*cp, max_batch), &cm_acc, &cm_acc_bytes);
    if (e != JN_OK) return e;
    cm.on = true; cm.cp = *cp; cm.hits = dHits; cm.grid = dGrid;
    return JN_OK;
  }

  // cp == nullptr: the scan only (dHits and dGrid must be null too); everything null detaches
  jn_status attach_subpix(int device, int max_batch, const jn_costmap_params* cp, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid) {
    const bool detach = !cp && !dBins && !dMeta && !dHits && !dGrid;
    if (!detach && (!dBins || !dMeta || (cp ? (!costmap_params_valid(cp) || !dHits || !dGrid) : (dHits || dGrid)))) return JN_ERR_INVALID;
    if (detach) { sx = Subpix(); return JN_OK; }
    const jn_status e = grow(device, subpix_scratch_bytes(cp, max_batch), &sx_scratch, &sx_bytes);
    if (e != JN_OK) return e;
    sx = Subpix();
    sx.on = true; sx.has_cp = cp != nullptr; if (cp) sx.cp = *cp;
    sx.bins = dBins; sx.meta = dMeta; sx.hits = dHits; sx.grid = dGrid;
    return JN_OK;
  }

  // fp == nullptr detaches; `native`: the format of the handle's maps (a jn_disp_format)
  jn_status attach_postfilter(int device, int max_batch, int W, int H, int native, const jn_postfilter_params* fp, uint32_t* dStats) {
    if (!fp) { pf = Postfilter(); return JN_OK; }
    if (!postfilter_params_valid(fp) || fp->format != native) return JN_ERR_INVALID;
    const jn_status e = grow(device, postfilter_scratch_bytes(*fp, max_batch, W, H, true), &pf_scratch, &pf_bytes);
    if (e != JN_OK) return e;
    pf.on = true; pf.fp = *fp; pf.stats = dStats;
    return JN_OK;
  }

  // Ahead of everything that consumes the matcher's map, on the batch's stream: the attached post-filter, in place.
  hipError_t launch_postfilter_in_place(hipStream_t st, int n, int16_t* dDisp, int W, int H) const {
    return pf.on ? launch_postfilter(st, pf.fp, n, dDisp, W, H, dDisp, pf.stats, pf_scratch) : hipSuccess;
  }

  // Behind a scan batch, on its stream: the costmap of the mono8 map and the bins the scan has just written, then the sub-pixel tail of the
  // matcher's own map (`native`, in `format`: a jn_disp_format) with the default min_q.  The only error is the costmap's clear.
  hipError_t launch(hipStream_t st, const jn_scan_params& sp, int n, const uint8_t* dDispU8, const uint8_t* dLut, const double* dBins,
                    const void* native, int format, int W, int H) const {
    if (cm.on) {
      const hipError_t e = launch_costmap(st, sp, cm.cp, n, dDispU8, dLut, W, H, dBins, static_cast<uint32_t*>(cm_acc), cm.hits, cm.grid);
      if (e != hipSuccess) return e;
    }
    if (sx.on) {
      jn_subpix_params fp;
      jn_subpix_params_default(&fp, format);
      launch_subpix(st, sp, sx.has_cp ? &sx.cp : nullptr, fp, n, native, W, H, sx.bins, sx.meta, sx.hits, sx.grid, sx_scratch);
    }
    return hipSuccess;
  }

  void release() {
    (void)hipFree(cm_acc); (void)hipFree(sx_scratch); (void)hipFree(pf_scratch);
    *this = NavTails();
  }
};

#ifdef __HIPCC__
// ---- device side -------------------------------------------------------------------------------------------------------------------
#define DEV static __device__ __forceinline__

struct NavGeom {                                                // jn_scan_params as the kernels take it (nav_geom)
  double Q[16], XR[9], XT[3];
  int ox, oy;
  double gp_h, gp_tan, gp_dist, fov, pi;
  int bins;
};
struct NavGrid {                                                // jn_costmap_params' grid
  double org_x, org_y, res;
  int cx, cy;
};

static NavGeom nav_geom(const jn_scan_params& sp) {
  NavGeom g;
  for (int i = 0; i < 16; i++) g.Q[i] = sp.Q[i];
  for (int i = 0; i < 9; i++) g.XR[i] = sp.XR[i];
  for (int i = 0; i < 3; i++) g.XT[i] = sp.XT[i];
  g.ox = sp.crop_offset_x; g.oy = sp.crop_offset_y;
  g.gp_h = sp.gp_height_thresh; g.gp_tan = tan(sp.gp_angle_thresh); g.gp_dist = sp.gp_dist_thresh;
  g.fov = sp.fov_deg; g.pi = sp.pi_approx; g.bins = sp.bins;
  return g;
}
static NavGrid nav_grid(const jn_costmap_params& cp) { return NavGrid{cp.origin_x, cp.origin_y, cp.resolution, cp.cells_x, cp.cells_y}; }

// pos = Q*[i+ox, j+oy, V2, 1]; cam = pos.xyz/pos.w; robot = XR*cam + XT (point_cloud.cpp:237-253).  V2: the disparity in pixels.
DEV bool nav_reproject(const NavGeom& g, int i, int j, double V2, double& X, double& Y, double& Z) {
  const double V0 = (double)(i + g.ox), V1 = (double)(j + g.oy);
  double pos[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    double a = __dmul_rn(g.Q[4 * r], V0);
    a = __dadd_rn(a, __dmul_rn(g.Q[4 * r + 1], V1));
    a = __dadd_rn(a, __dmul_rn(g.Q[4 * r + 2], V2));
    a = __dadd_rn(a, g.Q[4 * r + 3]);
    pos[r] = a;
  }
  if (pos[3] == 0.0) return false;
  const double cx = pos[0] / pos[3], cy = pos[1] / pos[3], cz = pos[2] / pos[3];
  double o[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double a = __dmul_rn(g.XR[3 * r], cx);
    a = __dadd_rn(a, __dmul_rn(g.XR[3 * r + 1], cy));
    a = __dadd_rn(a, __dmul_rn(g.XR[3 * r + 2], cz));
    o[r] = __dadd_rn(a, g.XT[r]);
  }
  X = o[0]; Y = o[1]; Z = o[2];
  return true;
}
DEV bool nav_is_ground(const NavGeom& g, double X, double Z) {   // point_cloud.cpp:128-137
  if (X < g.gp_dist) return Z < g.gp_h;
  return Z < __dadd_rn(g.gp_h, __dmul_rn(g.gp_tan, X - g.gp_dist));
}

// jn_costmap.h "cell": the index of the point's cell, -1 outside the grid or for a non-finite point.  (X, Y, Z by reference, as
// nav_reproject hands them out: the callers' code then compiles to what it was with this text written out in each kernel.)
DEV int nav_cell(const NavGrid& c, const double& X, const double& Y, const double& Z) {
  int cell = -1;
  if (isfinite(X) && isfinite(Y) && isfinite(Z)) {
    const double fx = floor((X - c.org_x) / c.res), fy = floor((Y - c.org_y) / c.res);
    if (fx >= 0. && fx < (double)c.cx && fy >= 0. && fy < (double)c.cy) cell = (int)fy * c.cx + (int)fx;
  }
  return cell;
}
// the scan bin of bearing th, before the conversion to int: inside the field of view when 0 <= kf < bins (point_cloud.cpp:254-263, as k_scan)
DEV double nav_bin(const NavGeom& g, double th) {
  const double deg = __dmul_rn(th, 180.) / g.pi;
  return floor(__dmul_rn((double)g.bins, __dadd_rn(g.fov / 2., -deg)) / g.fov);
}

// order-preserving map double -> uint64 so that integer atomics implement min / max of doubles of either sign
DEV unsigned long long nav_enc(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
DEV double nav_dec(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}

// Adds cnt to acc[cell] for every lane with `have`, equal cells of the wave combined first: the lanes of a wave are neighbouring columns
// of one image tile and mostly hold the SAME cell (an obstacle's face) — 64 same-address atomics would serialise in the L2.  The first
// kCombine distinct cells are summed across the wave and added once each by their first lane; what is left after that (a wave looking
// at many cells: far, fronto-parallel clutter) goes out lane by lane.  Called by the whole wave (convergent).
constexpr int kCombine = 4;
DEV void nav_wave_add(bool have, int cell, uint32_t cnt, uint32_t* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int it = 0; it < kCombine; it++) {
    const unsigned long long m = __ballot(have);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    const int key = __shfl(cell, leader);
    const bool mine = have && cell == key;
    uint32_t sum = mine ? cnt : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == leader) atomicAdd(&acc[key], sum);
    if (mine) have = false;
  }
  if (have) atomicAdd(&acc[cell], cnt);
}

// A disparity map's element type by format, and its value in 1/16 pixel (jn_ground.h "q" and "valid"; jn_subpix.h takes both over).
// jn_ground.h and jn_subpix.h each name the three formats.
static_assert((int)JN_DISP_F32 == (int)JN_GROUND_F32 && (int)JN_DISP_I16 == (int)JN_GROUND_I16 && (int)JN_DISP_I16_SUB == (int)JN_GROUND_I16_SUB,
              "one set of format values");
constexpr int kMaxQ = 16 * JN_GROUND_MAX_SIDE;
template <int FMT> struct DispElem { using T = int16_t; };
template <> struct DispElem<JN_DISP_F32> { using T = float; };
template <int FMT>
DEV bool disp_to_q(typename DispElem<FMT>::T v, int min_q, int& q) {
  if constexpr (FMT == JN_DISP_F32) {
    const float t = rintf(__fmul_rn(16.f, v));
    const bool ok = isfinite(v) && t >= (float)min_q && t <= (float)kMaxQ;
    q = ok ? (int)t : 0;
    return ok;
  } else {
    q = FMT == JN_DISP_I16 ? 16 * (int)v : (int)v;
    return q >= min_q && q <= kMaxQ;
  }
}
#endif  // __HIPCC__

}  // namespace jnav

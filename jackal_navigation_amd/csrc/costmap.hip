// costmap.hip — the robot-frame obstacle costmap (include/jn_costmap.h): its kernels, launchers and the synchronous C entry point.  Product code.
//
// No reference counterpart; the definition is in jn_costmap.h, its scalar restatement (the checker) in tests/.  hits and the occupied
// cells are integer results of individually rounded double arithmetic, so the bar for them is bit-exactness.
//
// The geometry (reprojection, ground model, cell of a point, bin of a bearing) and the wave-combined add are nav_tail.h's, shared with
// scan.hip and subpix.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nav_tail.h"

namespace jnav {
namespace {

struct CmDev {
  NavGeom g;
  NavGrid c;
  int min_hits;
};

// Accumulate: hits per cell of one batch into acc [n][cy][cx] u32 (cleared in stream order ahead of the launch).
// k_scan's shape: one thread per column, kCmRows rows, all of the thread's u8 / LUT loads requested together, a candidate mask, the
// reprojection only for candidates.  An obstacle is a near-vertical surface: consecutive rows of a column carry the same disparity and
// fall in the same cell, so a thread keeps (cell, count) in registers and emits one add per RUN of rows, not per pixel; the adds of a
// wave are combined (nav_wave_add).  The candidate loop is wave-uniform (it runs while any lane has rows left) so that the combining
// sees the whole wave.
constexpr int kCmRows = 16;
template <bool kFromCloud>
__global__ void __launch_bounds__(256) k_costmap_accumulate(CmDev s, const uint8_t* __restrict__ disp, const uint8_t* __restrict__ lut, int W, int H,
                                                            uint32_t* __restrict__ acc) {
  const int frame = blockIdx.z;
  const int i = blockIdx.x * 256 + threadIdx.x, j0 = blockIdx.y * kCmRows;
  const int jend = min(j0 + kCmRows, H);
  uint32_t* __restrict__ facc = acc + (size_t)frame * s.c.cx * s.c.cy;
  uint32_t u8pk[kCmRows / 4] = {};
  uint32_t cand = 0;
  if (i < W) {
    int dv[kCmRows];
#pragma unroll
    for (int r = 0; r < kCmRows; r++) dv[r] = disp[((size_t)frame * H + min(j0 + r, H - 1)) * W + i];
    uint32_t lt[kCmRows];
    if (!kFromCloud) {
#pragma unroll
      for (int r = 0; r < kCmRows; r++) lt[r] = reinterpret_cast<const uint16_t*>(lut)[(size_t)min(j0 + r, H - 1) * W + i];       // point_cloud.cpp:234
    }
#pragma unroll
    for (int r = 0; r < kCmRows; r++) {
      u8pk[r >> 2] |= (uint32_t)dv[r] << (8 * (r & 3));
      const bool c = kFromCloud ? dv[r] >= 2 : (dv[r] >= (int)(lt[r] & 0xFF) && dv[r] <= (int)(lt[r] >> 8));
      if (c && j0 + r < jend) cand |= 1u << r;
    }
  }
  int cur_cell = -1;
  uint32_t cur_cnt = 0;
  uint32_t mk = cand;
  while (__any(mk != 0u)) {
    bool flush = false;
    int fcell = 0;
    uint32_t fcnt = 0;
    if (mk) {
      const int rr = __ffs((int)mk) - 1, j = j0 + rr;
      mk &= mk - 1;
      const uint32_t w = rr < 8 ? (rr < 4 ? u8pk[0] : u8pk[1]) : (rr < 12 ? u8pk[2] : u8pk[3]);
      const int d = (int)((w >> (8 * (rr & 3))) & 255u);
      double X = 0, Y = 0, Z = 0;
      bool take = nav_reproject(s.g, i, j, (double)d, X, Y, Z);
      if (kFromCloud) take = take && !nav_is_ground(s.g, X, Z);                                   // :166-172
      int cell = -1;
      if (take) cell = nav_cell(s.c, X, Y, Z);
      if (cell == cur_cell) cur_cnt++;
      else {
        if (cur_cell >= 0) { flush = true; fcell = cur_cell; fcnt = cur_cnt; }
        cur_cell = cell; cur_cnt = 1;
      }
    }
    if (__any(flush)) nav_wave_add(flush, fcell, fcnt, facc);
  }
  nav_wave_add(cur_cell >= 0, cur_cell, cur_cnt, facc);
}

// Finish: one thread per cell and frame.  acc != nullptr: hits = min(acc, 65535) is written; acc == nullptr: hits is read (the merge's
// recomputation).  grid from hits and the frame's bins (jn_costmap.h).
__global__ void __launch_bounds__(256) k_costmap_finish(CmDev s, int n, const uint32_t* __restrict__ acc, uint16_t* __restrict__ hits,
                                                        const double* __restrict__ bins, int8_t* __restrict__ grid) {
  const int cells = s.c.cx * s.c.cy;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * cells) return;
  const int frame = (int)(t / cells), c = (int)(t - (long long)frame * cells);
  uint32_t h;
  if (acc) { h = min(acc[t], 65535u); hits[t] = (uint16_t)h; }
  else h = hits[t];
  int8_t g = -1;
  if (h >= (uint32_t)s.min_hits) g = 100;
  else if (bins) {
    const int iy = c / s.c.cx, ix = c - iy * s.c.cx;
    const double xc = __dadd_rn(s.c.org_x, __dmul_rn(__dadd_rn((double)ix, 0.5), s.c.res));
    const double yc = __dadd_rn(s.c.org_y, __dmul_rn(__dadd_rn((double)iy, 0.5), s.c.res));
    const double kf = nav_bin(s.g, atan2(yc, xc));
    if (kf >= 0 && kf < (double)s.g.bins) {
      const double b = bins[(size_t)frame * s.g.bins + (int)kf];
      const double r = sqrt(__dadd_rn(__dmul_rn(yc, yc), __dmul_rn(xc, xc)));
      if (b < JN_SCAN_EMPTY - 1 && __dadd_rn(r, s.c.res) <= b) g = 0;
    }
  }
  grid[t] = g;
}

// Cross-rig merge (comm.cpp): hits <-> the communicator's packed buffer, counts negated (exact) so that the scan's MIN all-reduce takes
// their maximum.  +inf, the identity a failed rank feeds the reduction, unpacks to 0 hits.
__global__ void __launch_bounds__(256) k_costmap_pack(long long count, uint16_t* __restrict__ hits, double* __restrict__ flat, int pack) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  if (pack) flat[i] = -(double)hits[i];
  else {
    const double v = -flat[i];
    hits[i] = (v >= 0. && v <= 65535.) ? (uint16_t)v : (uint16_t)(v > 65535. && v < INFINITY ? 65535 : 0);
  }
}

CmDev cm_to_dev(const jn_scan_params& sp, const jn_costmap_params& cp) { return CmDev{nav_geom(sp), nav_grid(cp), cp.min_hits}; }

}  // namespace

bool costmap_params_valid(const jn_costmap_params* cp) {
  return cp && std::isfinite(cp->origin_x) && std::isfinite(cp->origin_y) && std::isfinite(cp->resolution) && cp->resolution > 0. &&
         cp->cells_x >= 1 && cp->cells_x <= JN_COSTMAP_MAX_CELLS && cp->cells_y >= 1 && cp->cells_y <= JN_COSTMAP_MAX_CELLS &&
         cp->min_hits >= 1 && (cp->from_cloud == 0 || cp->from_cloud == 1);
}

size_t costmap_scratch_bytes(const jn_costmap_params& cp, int n) { return sizeof(uint32_t) * (size_t)n * cp.cells_x * cp.cells_y; }

void launch_costmap_finish(hipStream_t st, const jn_scan_params& sp, const jn_costmap_params& cp, int n, const uint32_t* acc, uint16_t* hits,
                           const double* bins, int8_t* grid) {
  const long long total = (long long)n * cp.cells_x * cp.cells_y;
  hipLaunchKernelGGL(k_costmap_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, cm_to_dev(sp, cp), n, acc, hits, bins, grid);
}

hipError_t launch_costmap(hipStream_t st, const jn_scan_params& sp, const jn_costmap_params& cp, int n, const uint8_t* disp, const uint8_t* lut,
                          int W, int H, const double* bins, uint32_t* acc, uint16_t* hits, int8_t* grid) {
  // the clear on the SAME stream: a null-stream memset is not ordered against a slot's non-blocking stream
  const hipError_t e = hipMemsetAsync(acc, 0, costmap_scratch_bytes(cp, n), st);
  if (e != hipSuccess) return e;
  const CmDev s = cm_to_dev(sp, cp);
  const dim3 g((W + 255) / 256, (H + kCmRows - 1) / kCmRows, n);
  if (cp.from_cloud) hipLaunchKernelGGL((k_costmap_accumulate<true>), g, dim3(256), 0, st, s, disp, lut, W, H, acc);
  else hipLaunchKernelGGL((k_costmap_accumulate<false>), g, dim3(256), 0, st, s, disp, lut, W, H, acc);
  launch_costmap_finish(st, sp, cp, n, acc, hits, bins, grid);
  return hipSuccess;
}

void launch_costmap_pack(hipStream_t st, long long count, uint16_t* hits, double* flat, bool pack) {
  hipLaunchKernelGGL(k_costmap_pack, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, count, hits, flat, pack ? 1 : 0);
}

}  // namespace jnav

using namespace jnav;

extern "C" {

void jn_costmap_params_default(jn_costmap_params* cp) {
  cp->origin_x = 0.0; cp->origin_y = -3.2; cp->resolution = 0.05;
  cp->cells_x = 128; cp->cells_y = 128; cp->min_hits = 3; cp->from_cloud = 0;
}

jn_status jn_obstacle_costmap(int32_t device, const jn_scan_params* sp, const jn_costmap_params* cp, int32_t n, const uint8_t* dDisp,
                              const uint8_t* dLut, int32_t W, int32_t H, const double* dBins, uint16_t* dHits, int8_t* dGrid) {
  if (!sp || !costmap_params_valid(cp) || !dDisp || !dHits || !dGrid || n < 1 || W < 1 || H < 1 || sp->bins < 1 || sp->bins > 1024 ||
      (!cp->from_cloud && !dLut))
    return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  void* acc = nullptr;
  HIP_TRY(thread_scratch(device, costmap_scratch_bytes(*cp, n), &acc));
  HIP_TRY(launch_costmap(nullptr, *sp, *cp, n, dDisp, dLut, W, H, dBins, static_cast<uint32_t*>(acc), dHits, dGrid));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // extern "C"

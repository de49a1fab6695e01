// subpix.hip — the sub-pixel navigation tail (include/jn_subpix.h): obstacle scan, costmap and point cloud from fractional disparities.
// Its kernels, launchers and the synchronous C entry points.  Product code.
//
// No reference counterpart; the definition is in jn_subpix.h, its scalar restatement (the checker) in tests/subpix_def.py.  The anchor
// of that header — bit-identity with jn_obstacle_scan_cloud, jn_obstacle_costmap(from_cloud = 1) and jn_point_cloud on integer maps —
// holds because the reprojection, the ground model, the cell and the bin of a point are nav_tail.h's own functions, the ones scan.hip and
// costmap.hip call, and the grid classification is costmap.hip's own finish kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "nav_tail.h"

namespace jnav {
namespace {

struct SpxDev {
  NavGeom g;
  NavGrid c;
  int min_q;
};

// bins [n][bins] (in the caller's dBins, as order-encoded uint64 until k_spx_finish), extrema [n][4], acc [n][cells] (may be null)
__global__ void __launch_bounds__(256) k_spx_init(long long total_bins, int n, long long total_cells, unsigned long long* __restrict__ gbins,
                                                  unsigned long long* __restrict__ gmeta, uint32_t* __restrict__ acc) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < total_bins) gbins[t] = ~0ull;
  if (t < (long long)n * 4) gmeta[t] = (t & 1) ? 0ull : ~0ull;                 // min slots start high, max slots low
  if (t < total_cells) acc[t] = 0u;
}

// The one pass over the pixels: format conversion, reprojection, ground test, bearing and range of every obstacle pixel, reduced into
// the frame's bins / extrema (and, kCostmap, its cell counts).
// k_scan's work shape: one thread per column, kSpxRows rows, the thread's loads requested together.  What differs: the rows are visited
// by the whole wave TOGETHER (the loop counter is wave-uniform, a row nobody needs is skipped by the wave), so that the cell counts can be
// combined across the wave (nav_wave_add is convergent) and the row's terms of the reprojection are the same in every lane.
// An obstacle is a near-vertical surface: consecutive rows of a column fall in the same bin and mostly in the same cell, so a thread keeps
// (bin, running minimum) and (cell, count) in registers and goes to the LDS / the accumulation grid once per RUN of rows.
constexpr int kSpxRows = 16;
template <int FMT, bool kCostmap>
__global__ void __launch_bounds__(256) k_spx_accumulate(SpxDev s, const void* __restrict__ disp_, int W, int H, unsigned long long* __restrict__ gbins,
                                                        unsigned long long* __restrict__ gmeta, uint32_t* __restrict__ acc) {
  using T = typename DispElem<FMT>::T;
  const T* __restrict__ disp = static_cast<const T*>(disp_);
  extern __shared__ unsigned long long lds[];      // [bins] + 4
  unsigned long long* lbins = lds;
  unsigned long long* lmeta = lds + s.g.bins;
  const int frame = blockIdx.z;
  for (int k = threadIdx.x; k < s.g.bins; k += 256) lbins[k] = ~0ull;
  if (threadIdx.x < 4) lmeta[threadIdx.x] = (threadIdx.x & 1) ? 0ull : ~0ull;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x, j0 = blockIdx.y * kSpxRows;
  int qv[kSpxRows];
  uint32_t cand = 0;
  if (i < W) {
    T raw[kSpxRows];
#pragma unroll
    for (int r = 0; r < kSpxRows; r++) raw[r] = disp[((size_t)frame * H + min(j0 + r, H - 1)) * W + i];
#pragma unroll
    for (int r = 0; r < kSpxRows; r++)
      if (disp_to_q<FMT>(raw[r], s.min_q, qv[r]) && j0 + r < H) cand |= 1u << r;
  } else {
#pragma unroll
    for (int r = 0; r < kSpxRows; r++) qv[r] = 0;
  }
  unsigned long long tmin = ~0ull, tmax = 0ull, rmin = ~0ull, rmax = 0ull;
  int cur_bin = -1;
  unsigned long long cur_min = ~0ull;
  int cur_cell = -1;
  uint32_t cur_cnt = 0;
  uint32_t* __restrict__ facc = kCostmap ? acc + (size_t)frame * s.c.cx * s.c.cy : nullptr;
#pragma unroll 1
  for (int r = 0; r < kSpxRows; r++) {
    const bool on = (cand >> r) & 1u;
    if (!__any(on)) continue;                                                                     // wave-uniform
    bool flush = false;
    int fcell = 0;
    uint32_t fcnt = 0;
    if (on) {
      int q = qv[0];                                                                              // r is uniform: a chain of selects, no indexed registers
#pragma unroll
      for (int k = 1; k < kSpxRows; k++) q = (r == k) ? qv[k] : q;
      double X = 0, Y = 0, Z = 0;
      const bool take = nav_reproject(s.g, i, j0 + r, __dmul_rn((double)q, 0.0625), X, Y, Z) && !nav_is_ground(s.g, X, Z);   // q / 16.0, exact
      if (take) {
        const double th = atan2(Y, X);
        const double rg = sqrt(__dadd_rn(__dmul_rn(Y, Y), __dmul_rn(X, X)));
        const unsigned long long et = nav_enc(th), er = nav_enc(rg);
        tmin = min(tmin, et); tmax = max(tmax, et); rmin = min(rmin, er); rmax = max(rmax, er);
        const double kf = nav_bin(s.g, th);
        if (kf >= 0 && kf < (double)s.g.bins) {
          const int k = (int)kf;
          if (k != cur_bin) {
            if (cur_bin >= 0) atomicMin(&lbins[cur_bin], cur_min);
            cur_bin = k; cur_min = er;
          } else cur_min = min(cur_min, er);
        }
      }
      if (kCostmap) {
        int cell = -1;
        if (take) cell = nav_cell(s.c, X, Y, Z);
        if (cell == cur_cell) cur_cnt++;
        else {
          if (cur_cell >= 0) { flush = true; fcell = cur_cell; fcnt = cur_cnt; }
          cur_cell = cell; cur_cnt = 1;
        }
      }
    }
    if (kCostmap) { if (__any(flush)) nav_wave_add(flush, fcell, fcnt, facc); }
  }
  if (cur_bin >= 0) atomicMin(&lbins[cur_bin], cur_min);
  if (kCostmap) nav_wave_add(cur_cell >= 0, cur_cell, cur_cnt, facc);
  // extrema: butterfly inside the wave, then one LDS atomic per wave — skipped by the waves in which no pixel was an obstacle
  if (__ballot(tmin != ~0ull) != 0ull) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      tmin = min(tmin, __shfl_xor(tmin, off)); tmax = max(tmax, __shfl_xor(tmax, off));
      rmin = min(rmin, __shfl_xor(rmin, off)); rmax = max(rmax, __shfl_xor(rmax, off));
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(&lmeta[0], tmin); atomicMax(&lmeta[1], tmax); atomicMin(&lmeta[2], rmin); atomicMax(&lmeta[3], rmax); }
  }
  __syncthreads();
  // one device-scope atomic per touched bin and workgroup
  for (int k = threadIdx.x; k < s.g.bins; k += 256)
    if (lbins[k] != ~0ull) atomicMin(&gbins[(size_t)frame * s.g.bins + k], lbins[k]);
  if (threadIdx.x < 4) {
    const unsigned long long x = lmeta[threadIdx.x];
    if (threadIdx.x & 1) { if (x != 0ull) atomicMax(&gmeta[frame * 4 + threadIdx.x], x); }
    else { if (x != ~0ull) atomicMin(&gmeta[frame * 4 + threadIdx.x], x); }
  }
}

// encoded minima -> doubles in place (JN_SCAN_EMPTY where nothing fell), extrema -> dMeta (point_cloud.cpp:219-220 where untouched)
__global__ void __launch_bounds__(256) k_spx_finish(long long total_bins, int n, unsigned long long* __restrict__ gbins,
                                                    const unsigned long long* __restrict__ gmeta, double* __restrict__ meta) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < total_bins) {
    const unsigned long long k = gbins[t];
    reinterpret_cast<double*>(gbins)[t] = (k == ~0ull) ? JN_SCAN_EMPTY : nav_dec(k);
  }
  if (t < (long long)n * 4) {
    const unsigned long long k = gmeta[t];
    const double init[4] = {400., -400., 1e9, -500.};
    const bool untouched = (t & 1) ? (k == 0ull) : (k == ~0ull);
    meta[t] = untouched ? init[t & 3] : nav_dec(k);
  }
}

// Point cloud: k_pc_*'s shape (counts per column, exclusive scan, ordered write), over valid pixels.  col_count: [W + 1] int64.
template <int FMT>
__global__ void __launch_bounds__(256) k_spx_pc_count(const void* __restrict__ disp_, int min_q, int W, int H, long long* __restrict__ col_count) {
  const typename DispElem<FMT>::T* __restrict__ disp = static_cast<const typename DispElem<FMT>::T*>(disp_);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W) return;
  int c = 0, q;
  for (int j = 0; j < H; j++) c += disp_to_q<FMT>(disp[(size_t)j * W + i], min_q, q) ? 1 : 0;
  col_count[i + 1] = c;
  if (i == 0) col_count[0] = 0;
}
__global__ void k_spx_pc_scan(int W, long long* col_count) {   // tiny: one thread, W <= a few thousand
  if (threadIdx.x == 0 && blockIdx.x == 0) for (int i = 1; i <= W; i++) col_count[i] += col_count[i - 1];
}
template <int FMT>
__global__ void __launch_bounds__(256) k_spx_pc_scatter(SpxDev s, const void* __restrict__ disp_, int W, int H,
                                                        const long long* __restrict__ col_count, float* __restrict__ xyz) {
  const typename DispElem<FMT>::T* __restrict__ disp = static_cast<const typename DispElem<FMT>::T*>(disp_);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W) return;
  long long o = col_count[i];
  for (int j = 0; j < H; j++) {
    int q;
    if (!disp_to_q<FMT>(disp[(size_t)j * W + i], s.min_q, q)) continue;
    double X, Y, Z;
    if (!nav_reproject(s.g, i, j, __dmul_rn((double)q, 0.0625), X, Y, Z)) { X = Y = Z = 0; }
    xyz[3 * o] = (float)X; xyz[3 * o + 1] = (float)Y; xyz[3 * o + 2] = (float)Z; o++;
  }
}

SpxDev spx_to_dev(const jn_scan_params& sp, const jn_costmap_params* cp, const jn_subpix_params& fp) {
  return SpxDev{nav_geom(sp), cp ? nav_grid(*cp) : NavGrid{0., 0., 1., 0, 0}, fp.min_q};
}

template <bool kCostmap>
void spx_launch_accumulate(hipStream_t st, const SpxDev& s, int format, int n, const void* disp, int W, int H, unsigned long long* gbins,
                           unsigned long long* gmeta, uint32_t* acc) {
  const dim3 g((W + 255) / 256, (H + kSpxRows - 1) / kSpxRows, n);
  const size_t lds = (s.g.bins + 4) * sizeof(unsigned long long);
  if (format == JN_DISP_F32) hipLaunchKernelGGL((k_spx_accumulate<JN_DISP_F32, kCostmap>), g, dim3(256), lds, st, s, disp, W, H, gbins, gmeta, acc);
  else if (format == JN_DISP_I16) hipLaunchKernelGGL((k_spx_accumulate<JN_DISP_I16, kCostmap>), g, dim3(256), lds, st, s, disp, W, H, gbins, gmeta, acc);
  else hipLaunchKernelGGL((k_spx_accumulate<JN_DISP_I16_SUB, kCostmap>), g, dim3(256), lds, st, s, disp, W, H, gbins, gmeta, acc);
}

}  // namespace

bool subpix_params_valid(const jn_subpix_params* fp) {
  return fp && (fp->format == JN_DISP_F32 || fp->format == JN_DISP_I16 || fp->format == JN_DISP_I16_SUB) && fp->min_q >= 0 && fp->min_q <= kMaxQ;
}

size_t subpix_scratch_bytes(const jn_costmap_params* cp, int n) {
  return sizeof(unsigned long long) * 4 * (size_t)n + (cp ? costmap_scratch_bytes(*cp, n) : 0);
}

void launch_subpix(hipStream_t st, const jn_scan_params& sp, const jn_costmap_params* cp, const jn_subpix_params& fp, int n, const void* disp,
                   int W, int H, double* bins, double* meta, uint16_t* hits, int8_t* grid, void* scratch) {
  const SpxDev s = spx_to_dev(sp, cp, fp);
  unsigned long long* gbins = reinterpret_cast<unsigned long long*>(bins);
  unsigned long long* gmeta = static_cast<unsigned long long*>(scratch);
  uint32_t* acc = cp ? reinterpret_cast<uint32_t*>(gmeta + 4 * (size_t)n) : nullptr;
  const long long total_bins = (long long)n * sp.bins, total_cells = cp ? (long long)n * cp->cells_x * cp->cells_y : 0;
  const long long m = std::max(std::max(total_bins, total_cells), (long long)n * 4);
  // everything the pass accumulates into is initialised on the SAME stream (a null-stream memset is not ordered against a slot's stream)
  hipLaunchKernelGGL(k_spx_init, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, total_bins, n, total_cells, gbins, gmeta, acc);
  if (cp) spx_launch_accumulate<true>(st, s, fp.format, n, disp, W, H, gbins, gmeta, acc);
  else spx_launch_accumulate<false>(st, s, fp.format, n, disp, W, H, gbins, gmeta, acc);
  hipLaunchKernelGGL(k_spx_finish, dim3((unsigned)((std::max(total_bins, (long long)n * 4) + 255) / 256)), dim3(256), 0, st, total_bins, n, gbins, gmeta, meta);
  if (cp) launch_costmap_finish(st, sp, *cp, n, acc, hits, bins, grid);      // costmap.hip's saturate-and-classify, from the bins just written
}

void launch_subpix_point_cloud(hipStream_t st, const jn_scan_params& sp, const jn_subpix_params& fp, const void* disp, int W, int H, float* xyz,
                               long long* col_count) {
  const SpxDev s = spx_to_dev(sp, nullptr, fp);
  const dim3 g((W + 255) / 256);
  if (fp.format == JN_DISP_F32) hipLaunchKernelGGL((k_spx_pc_count<JN_DISP_F32>), g, dim3(256), 0, st, disp, fp.min_q, W, H, col_count);
  else if (fp.format == JN_DISP_I16) hipLaunchKernelGGL((k_spx_pc_count<JN_DISP_I16>), g, dim3(256), 0, st, disp, fp.min_q, W, H, col_count);
  else hipLaunchKernelGGL((k_spx_pc_count<JN_DISP_I16_SUB>), g, dim3(256), 0, st, disp, fp.min_q, W, H, col_count);
  hipLaunchKernelGGL(k_spx_pc_scan, dim3(1), dim3(64), 0, st, W, col_count);
  if (fp.format == JN_DISP_F32) hipLaunchKernelGGL((k_spx_pc_scatter<JN_DISP_F32>), g, dim3(256), 0, st, s, disp, W, H, col_count, xyz);
  else if (fp.format == JN_DISP_I16) hipLaunchKernelGGL((k_spx_pc_scatter<JN_DISP_I16>), g, dim3(256), 0, st, s, disp, W, H, col_count, xyz);
  else hipLaunchKernelGGL((k_spx_pc_scatter<JN_DISP_I16_SUB>), g, dim3(256), 0, st, s, disp, W, H, col_count, xyz);
}

}  // namespace jnav

using namespace jnav;

namespace {

jn_status spx_sync_call(int32_t device, const jn_scan_params* sp, const jn_costmap_params* cp, const jn_subpix_params* fp, int32_t n, const void* dDisp,
                        int32_t W, int32_t H, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid) {
  HIP_TRY(hipSetDevice(device));
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, subpix_scratch_bytes(cp, n), &scratch));
  launch_subpix(nullptr, *sp, cp, *fp, n, dDisp, W, H, dBins, dMeta, dHits, dGrid, scratch);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // namespace

extern "C" {

void jn_subpix_params_default(jn_subpix_params* fp, int32_t format) {
  fp->format = format; fp->min_q = 32;
}

jn_status jn_subpix_scan(int32_t device, const jn_scan_params* sp, const jn_subpix_params* fp, int32_t n, const void* dDisp, int32_t W, int32_t H,
                         double* dBins, double* dMeta) {
  if (!sp || !subpix_params_valid(fp) || !dDisp || !dBins || !dMeta || n < 1 || W < 1 || H < 1 || sp->bins < 1 || sp->bins > 1024) return JN_ERR_INVALID;
  return spx_sync_call(device, sp, nullptr, fp, n, dDisp, W, H, dBins, dMeta, nullptr, nullptr);
}

jn_status jn_subpix_costmap(int32_t device, const jn_scan_params* sp, const jn_costmap_params* cp, const jn_subpix_params* fp, int32_t n,
                            const void* dDisp, int32_t W, int32_t H, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid) {
  if (!sp || !costmap_params_valid(cp) || !subpix_params_valid(fp) || !dDisp || !dBins || !dMeta || !dHits || !dGrid || n < 1 || W < 1 || H < 1 ||
      sp->bins < 1 || sp->bins > 1024)
    return JN_ERR_INVALID;
  return spx_sync_call(device, sp, cp, fp, n, dDisp, W, H, dBins, dMeta, dHits, dGrid);
}

jn_status jn_subpix_point_cloud(int32_t device, const jn_scan_params* sp, const jn_subpix_params* fp, const void* dDisp, int32_t W, int32_t H,
                                float* dXyz, int64_t* count) {
  if (!sp || !subpix_params_valid(fp) || !dDisp || !dXyz || !count || W < 1 || H < 1) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, sizeof(long long) * ((size_t)W + 1), &scratch));
  long long* cols = static_cast<long long*>(scratch);
  launch_subpix_point_cloud(nullptr, *sp, *fp, dDisp, W, H, dXyz, cols);
  long long total = 0;
  HIP_TRY(hipMemcpy(&total, cols + W, sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  *count = total;
  return JN_OK;
}

}  // extern "C"

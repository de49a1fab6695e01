// localmap.hip — the odometry-fused local obstacle map (include/jn_localmap.h): a rolling int16 log-odds grid in a fixed frame, fed by
// disparity maps and poses.  Its kernels, the handle and the C entry points.  Product code.
//
// No reference counterpart; the definition is in jn_localmap.h, its scalar restatement (the checker) in tests/localmap_def.py.  The
// conversion, the reprojection, the ground model and the cell of a point are nav_tail.h's own functions, the ones costmap.hip and subpix.hip
// call: the header's anchor (obstacle counts == jn_subpix_costmap's hits under the zero pose) holds because of that.
//
// Three kernels.
//   k_lm_accumulate  one pass over the pixels of a batch: every valid pixel is counted into its frame's obstacle or floor plane of the
//                    count scratch [n][2][cells] u32.  See the kernel for the shape of the combine.
//   k_lm_fuse        one thread per window cell: the n frames' counts in index order, one read and one write of L.
//   k_lm_shift       recentre: L copied into the handle's second buffer at the new window's offset, zeros where cells enter; the two
//                    buffers then swap.  A window is at most 512 x 512 int16 (512 KB): the copy costs less than the bookkeeping of a
//                    toroidal store would in every other kernel, and L stays in window order for all of them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>
#include "nav_tail.h"
#include "../../include/jn_localmap.h"

namespace jnav {
namespace {

constexpr int kLmMaxBatch = 256;
constexpr double kLmMaxIndex = 1073741824.0;      // 2^30: |x / resolution| of a pose or a window centre

struct LmDev {
  NavGeom g;
  NavGrid c;                                      // the window: origin = g0 * resolution
  int min_q;
};
struct LmPose { double c, s, x, y; };             // cos / sin of theta taken on the host

// Adds cnt to acc[key] for every lane with `have`, RUNS of equal keys in neighbouring lanes combined first: one add per run, by its first
// lane.  The lanes of a wave are neighbouring columns of one image row band.  A floor row has constant depth and walks ACROSS the cells,
// a run of lanes per cell (near the robot a 5 cm cell is tens of pixels wide); an obstacle face gives the same picture.  nav_wave_add,
// which sums the first four distinct cells of a wave, leaves a floor row's other cells to one atomic per lane; here the number of atomics
// is the number of runs whatever the number of distinct cells.
// Run heads by a ballot on "my key differs from my left neighbour's"; the run's sum from an inclusive prefix sum over the wave (the
// prefix at the run's last lane minus the prefix in front of the head).  Called by the whole wave (convergent).
DEV void lm_wave_add_runs(bool have, int key, uint32_t cnt, uint32_t* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  const int k = have ? key : -1;
  const int left = __shfl_up(k, 1);
  const bool head = lane == 0 || k != left;
  const unsigned long long heads = __ballot(head);
  const uint32_t mine = have ? cnt : 0u;
  uint32_t pre = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(pre, off);
    if (lane >= off) pre += t;
  }
  const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1));
  const int last = above ? lane + __ffsll((long long)above) - 1 : 63;              // the lane in front of the next head
  const uint32_t end = __shfl(pre, last);
  if (head && have) atomicAdd(&acc[key], end - pre + mine);
}

// The one pass over the pixels.  k_spx_accumulate's work shape: one thread per column, kLmRows rows, the thread's loads requested
// together, the rows visited by the whole wave TOGETHER (a wave-uniform loop, a row nobody needs is skipped).  What differs is the load:
// every valid pixel counts, and most of them are floor.
// Two combines, one after the other.  DOWN the column, in registers: a thread keeps (key, count) and emits one record per RUN of rows with
// one key (key = class * cells + cell) — an obstacle face is a run of a column's rows, and so is the floor near the robot, where the rows
// of one 5 cm cell are a dozen image rows apart.  ACROSS the lanes: the records a wave emits at one row are combined by lm_wave_add_runs.
// A floor cell's boundary in depth crosses a row band at the same row in neighbouring columns, so the records of a cell leave the lanes
// together, as one run.
constexpr int kLmRows = 16;
template <int FMT>
__global__ void __launch_bounds__(256) k_lm_accumulate(LmDev s, const LmPose* __restrict__ poses, const void* __restrict__ disp_, int W, int H,
                                                       uint32_t* __restrict__ acc) {
  using T = typename DispElem<FMT>::T;
  const T* __restrict__ disp = static_cast<const T*>(disp_);
  const int frame = blockIdx.z;
  const int cells = s.c.cx * s.c.cy;
  const LmPose p = poses[frame];                                                                  // uniform: scalar loads
  const int i = blockIdx.x * 256 + threadIdx.x, j0 = blockIdx.y * kLmRows;
  int qv[kLmRows];
  uint32_t cand = 0;
  if (i < W) {
    T raw[kLmRows];
#pragma unroll
    for (int r = 0; r < kLmRows; r++) raw[r] = disp[((size_t)frame * H + min(j0 + r, H - 1)) * W + i];
#pragma unroll
    for (int r = 0; r < kLmRows; r++)
      if (disp_to_q<FMT>(raw[r], s.min_q, qv[r]) && j0 + r < H) cand |= 1u << r;
  } else {
#pragma unroll
    for (int r = 0; r < kLmRows; r++) qv[r] = 0;
  }
  int cur_key = -1;
  uint32_t cur_cnt = 0;
  uint32_t* __restrict__ facc = acc + (size_t)frame * 2 * cells;
#pragma unroll 1
  for (int r = 0; r < kLmRows; r++) {
    const bool on = (cand >> r) & 1u;
    if (!__any(on)) continue;                                                                     // wave-uniform
    bool flush = false;
    int fkey = 0;
    uint32_t fcnt = 0;
    if (on) {
      int q = qv[0];                                                                              // r is uniform: a chain of selects, no indexed registers
#pragma unroll
      for (int k = 1; k < kLmRows; k++) q = (r == k) ? qv[k] : q;
      double X = 0, Y = 0, Z = 0;
      int key = -1;
      if (nav_reproject(s.g, i, j0 + r, __dmul_rn((double)q, 0.0625), X, Y, Z)) {                 // q / 16.0, exact
        const bool floor_px = nav_is_ground(s.g, X, Z);
        const double Xw = __dadd_rn(__dsub_rn(__dmul_rn(p.c, X), __dmul_rn(p.s, Y)), p.x);
        const double Yw = __dadd_rn(__dadd_rn(__dmul_rn(p.s, X), __dmul_rn(p.c, Y)), p.y);
        const int cell = nav_cell(s.c, Xw, Yw, Z);
        if (cell >= 0) key = (floor_px ? cells : 0) + cell;
      }
      if (key == cur_key) cur_cnt++;
      else {
        if (cur_key >= 0) { flush = true; fkey = cur_key; fcnt = cur_cnt; }
        cur_key = key; cur_cnt = 1;
      }
    }
    if (__any(flush)) lm_wave_add_runs(flush, fkey, fcnt, facc);
  }
  lm_wave_add_runs(cur_key >= 0, cur_key, cur_cnt, facc);
}

struct LmFuse {
  int cells, n;
  int min_hits, min_floor, l_hit, l_miss, l_min, l_max;
};

// One thread per window cell: the frames' saturated counts in index order (jn_localmap.h "state"), L read once and written once.
// obst / floor_out [n][cells] u16 may be null.
__global__ void __launch_bounds__(256) k_lm_fuse(LmFuse f, const uint32_t* __restrict__ acc, int16_t* __restrict__ L, uint16_t* __restrict__ obst,
                                                 uint16_t* __restrict__ floor_out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= f.cells) return;
  int l = L[c];
#pragma unroll 4
  for (int k = 0; k < f.n; k++) {
    const uint32_t o = min(acc[((size_t)k * 2) * f.cells + c], 65535u);
    const uint32_t g = min(acc[((size_t)k * 2 + 1) * f.cells + c], 65535u);
    if (obst) obst[(size_t)k * f.cells + c] = (uint16_t)o;
    if (floor_out) floor_out[(size_t)k * f.cells + c] = (uint16_t)g;
    if (o >= (uint32_t)f.min_hits) l = min(l + f.l_hit, f.l_max);
    else if (g >= (uint32_t)f.min_floor) l = max(l - f.l_miss, f.l_min);
  }
  L[c] = (int16_t)l;
}

// dst[iy][ix] = src[iy + dy][ix + dx] where that cell exists in the old window, else 0
__global__ void __launch_bounds__(256) k_lm_shift(int cx, int cy, int dx, int dy, const int16_t* __restrict__ src, int16_t* __restrict__ dst) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cx * cy) return;
  const int iy = c / cx, ix = c - iy * cx;
  const int sx = ix + dx, sy = iy + dy;
  dst[c] = (sx >= 0 && sx < cx && sy >= 0 && sy < cy) ? src[sy * cx + sx] : (int16_t)0;
}

__global__ void __launch_bounds__(256) k_lm_read(int cells, int occ, int fre, const int16_t* __restrict__ L, int16_t* __restrict__ lo,
                                                 int8_t* __restrict__ grid) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int l = L[c];
  if (lo) lo[c] = (int16_t)l;
  if (grid) grid[c] = l >= occ ? (int8_t)100 : (l <= fre ? (int8_t)0 : (int8_t)-1);
}

bool lm_params_valid(const jn_localmap_params* p) {
  return p && std::isfinite(p->resolution) && p->resolution > 0. && p->cells_x >= 1 && p->cells_x <= JN_COSTMAP_MAX_CELLS && p->cells_y >= 1 &&
         p->cells_y <= JN_COSTMAP_MAX_CELLS && p->min_hits >= 1 && p->min_floor >= 1 && p->l_hit >= 1 && p->l_hit <= 32767 && p->l_miss >= 1 &&
         p->l_miss <= 32767 && p->l_min >= -32768 && p->l_min < 0 && p->l_max > 0 && p->l_max <= 32767 && p->occ_thresh > 0 &&
         p->occ_thresh <= 32767 && p->free_thresh < 0 && p->free_thresh >= -32768 &&
         (p->format == JN_DISP_F32 || p->format == JN_DISP_I16 || p->format == JN_DISP_I16_SUB) && p->min_q >= 0 && p->min_q <= kMaxQ;
}

// a coordinate whose cell index stays far inside int64 / exact in double
bool lm_coord_valid(double v, double res) { return std::isfinite(v) && std::fabs(v / res) <= kLmMaxIndex; }

}  // namespace
}  // namespace jnav

using namespace jnav;

struct jn_localmap {
  jn_localmap_params p;
  int device = 0, max_batch = 0, cells = 0;
  int64_t g0[2] = {0, 0};
  int16_t* L = nullptr;            // the state, window order
  int16_t* L2 = nullptr;           // the recentre's target; swapped with L
  uint32_t* acc = nullptr;         // [max_batch][2][cells]
  LmPose* d_poses = nullptr;       // [max_batch]
  std::vector<LmPose> h_poses;
};

namespace {

void lm_centre_on(jn_localmap* h, double x, double y, int64_t g[2]) {
  g[0] = (int64_t)std::floor(x / h->p.resolution) - h->p.cells_x / 2;
  g[1] = (int64_t)std::floor(y / h->p.resolution) - h->p.cells_y / 2;
}

void lm_free(jn_localmap* h) {
  (void)hipFree(h->L); (void)hipFree(h->L2); (void)hipFree(h->acc); (void)hipFree(h->d_poses);
  delete h;
}

}  // namespace

extern "C" {

void jn_localmap_params_default(jn_localmap_params* p, int32_t format) {
  p->resolution = 0.05; p->cells_x = 256; p->cells_y = 256;
  p->min_hits = 3; p->min_floor = 3;
  p->l_hit = 4; p->l_miss = 1; p->l_min = -8; p->l_max = 16;            // untuned guesses (jn_localmap.h)
  p->occ_thresh = 4; p->free_thresh = -2;
  p->format = format; p->min_q = 32;
}

jn_status jn_localmap_create(const jn_localmap_params* p, int32_t max_batch, int32_t device, jn_localmap** out) {
  if (out) *out = nullptr;
  if (!lm_params_valid(p) || !out || max_batch < 1 || max_batch > kLmMaxBatch) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  jn_localmap* h = new (std::nothrow) jn_localmap();
  if (!h) return JN_ERR_INTERNAL;
  h->p = *p; h->device = device; h->max_batch = max_batch; h->cells = p->cells_x * p->cells_y;
  h->h_poses.resize(max_batch);
  const size_t lbytes = sizeof(int16_t) * (size_t)h->cells;
  if (hipMalloc(&h->L, lbytes) != hipSuccess || hipMalloc(&h->L2, lbytes) != hipSuccess ||
      hipMalloc(&h->acc, sizeof(uint32_t) * 2 * (size_t)h->cells * max_batch) != hipSuccess ||
      hipMalloc(&h->d_poses, sizeof(LmPose) * (size_t)max_batch) != hipSuccess || hipMemsetAsync(h->L, 0, lbytes, nullptr) != hipSuccess ||
      hipStreamSynchronize(nullptr) != hipSuccess) {
    lm_free(h);
    return JN_ERR_NO_DEVICE;
  }
  lm_centre_on(h, 0., 0., h->g0);
  *out = h;
  return JN_OK;
}

void jn_localmap_destroy(jn_localmap* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  lm_free(h);
}

jn_status jn_localmap_reset(jn_localmap* h) {
  if (!h) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemsetAsync(h->L, 0, sizeof(int16_t) * (size_t)h->cells, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  lm_centre_on(h, 0., 0., h->g0);
  return JN_OK;
}

jn_status jn_localmap_recenter(jn_localmap* h, double x, double y) {
  if (!h || !lm_coord_valid(x, h->p.resolution) || !lm_coord_valid(y, h->p.resolution)) return JN_ERR_INVALID;
  int64_t g[2];
  lm_centre_on(h, x, y, g);
  if (g[0] == h->g0[0] && g[1] == h->g0[1]) return JN_OK;
  HIP_TRY(hipSetDevice(h->device));
  // a move of a whole window or more empties it: any shift beyond the window does what the exact one does
  const int64_t lim = JN_COSTMAP_MAX_CELLS;
  const int dx = (int)std::max(-lim, std::min(lim, g[0] - h->g0[0])), dy = (int)std::max(-lim, std::min(lim, g[1] - h->g0[1]));
  hipLaunchKernelGGL(k_lm_shift, dim3((unsigned)((h->cells + 255) / 256)), dim3(256), 0, nullptr, h->p.cells_x, h->p.cells_y, dx, dy, h->L, h->L2);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  std::swap(h->L, h->L2);
  h->g0[0] = g[0]; h->g0[1] = g[1];
  return JN_OK;
}

jn_status jn_localmap_window(const jn_localmap* h, int64_t g0[2], double origin[2]) {
  if (!h) return JN_ERR_INVALID;
  if (g0) { g0[0] = h->g0[0]; g0[1] = h->g0[1]; }
  if (origin) { origin[0] = (double)h->g0[0] * h->p.resolution; origin[1] = (double)h->g0[1] * h->p.resolution; }
  return JN_OK;
}

jn_status jn_localmap_update(jn_localmap* h, const jn_scan_params* sp, int32_t n, const jn_pose2d* poses, const void* dDisp, int32_t W, int32_t H,
                             uint16_t* dObst, uint16_t* dFloor) {
  if (!h || !sp || !poses || !dDisp || n < 1 || n > h->max_batch || W < 1 || H < 1) return JN_ERR_INVALID;
  for (int f = 0; f < n; f++)
    if (!lm_coord_valid(poses[f].x, h->p.resolution) || !lm_coord_valid(poses[f].y, h->p.resolution) || !std::isfinite(poses[f].theta)) return JN_ERR_INVALID;
  for (int f = 0; f < n; f++) h->h_poses[f] = LmPose{std::cos(poses[f].theta), std::sin(poses[f].theta), poses[f].x, poses[f].y};
  HIP_TRY(hipSetDevice(h->device));
  const jn_localmap_params& p = h->p;
  LmDev s;
  s.g = nav_geom(*sp);
  s.c = NavGrid{(double)h->g0[0] * p.resolution, (double)h->g0[1] * p.resolution, p.resolution, p.cells_x, p.cells_y};
  s.min_q = p.min_q;
  // the poses, the clear of the counts and the kernels on ONE stream, in order
  HIP_TRY(hipMemcpyAsync(h->d_poses, h->h_poses.data(), sizeof(LmPose) * (size_t)n, hipMemcpyHostToDevice, nullptr));
  HIP_TRY(hipMemsetAsync(h->acc, 0, sizeof(uint32_t) * 2 * (size_t)h->cells * n, nullptr));
  const dim3 g((W + 255) / 256, (H + kLmRows - 1) / kLmRows, n);
  if (p.format == JN_DISP_F32) hipLaunchKernelGGL((k_lm_accumulate<JN_DISP_F32>), g, dim3(256), 0, nullptr, s, h->d_poses, dDisp, W, H, h->acc);
  else if (p.format == JN_DISP_I16) hipLaunchKernelGGL((k_lm_accumulate<JN_DISP_I16>), g, dim3(256), 0, nullptr, s, h->d_poses, dDisp, W, H, h->acc);
  else hipLaunchKernelGGL((k_lm_accumulate<JN_DISP_I16_SUB>), g, dim3(256), 0, nullptr, s, h->d_poses, dDisp, W, H, h->acc);
  const LmFuse fu{h->cells, n, p.min_hits, p.min_floor, p.l_hit, p.l_miss, p.l_min, p.l_max};
  hipLaunchKernelGGL(k_lm_fuse, dim3((unsigned)((h->cells + 255) / 256)), dim3(256), 0, nullptr, fu, h->acc, h->L, dObst, dFloor);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

jn_status jn_localmap_read(const jn_localmap* h, int16_t* dLogOdds, int8_t* dGrid) {
  if (!h || (!dLogOdds && !dGrid)) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_lm_read, dim3((unsigned)((h->cells + 255) / 256)), dim3(256), 0, nullptr, h->cells, h->p.occ_thresh, h->p.free_thresh, h->L,
                     dLogOdds, dGrid);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // extern "C"

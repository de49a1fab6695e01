// route.hip — the cost-to-go field (include/jn_route.h): the least cost of a path through free space from every cell of a clearance field
// to a goal, the arc rollout of plan.hip scored by it, and the host pieces (goal cell, choice, path).  Product code.
//
// No reference counterpart; the definition is in jn_route.h, its scalar restatement (Dijkstra with a heap: the checker) in
// tests/route_def.py.  The field is a shortest-path relaxation over u16 values: any schedule that relaxes to a fixed point gives the
// defined answer, and the kernels use that freedom.
//
// What is relaxed is not g but t(m) = pen(m) + g(m), the cost of a path that ENTERS m (65535 where that is above 65534 or m is not
// passable or not reached): then a cell's update needs only its own penalty bit — t(c) = pen(c) + min over the 8 neighbours of
// w + t(m) — and g(c) = min of w + t(m) is one last pull from the settled neighbours, which is the header's formula word for word.  A
// t above 65534 cannot contribute to any sum that survives the cut, so saturating it loses nothing.
//
// One workgroup relaxes a rectangle (a whole grid, or a tile of one) in LDS: t as u16 with a one-cell border and a row pitch of an odd
// number of dwords (lanes on consecutive rows fall on different banks), the passable and the near bits as two bit planes (odd words per
// row, for the same reason).  A ROUND is four sweeps — every row left to right and back, one thread per row, then every column down and
// up, one thread per column — each cell relaxed in place against all 8 neighbours with the three cells of the next column read ahead
// into registers.  A sweep carries a value along a whole straight corridor, so the rounds follow the number of TURNS of the longest
// path, not its length.  Rows and columns are separated by a barrier (a cell has one writer at a time: values only fall); a round in
// which no thread lowered anything ends the loop, through an LDS flag read into a scalar.  Every round settles at least the next cell in
// the order of the true values, so the loop ends after at most cells + 1 rounds.
//
// Two forms (the switch: rt_whole_fits — does the grid with its border and bit planes fit one CU's 160 KB of LDS; 256 x 256, the local
// map's default, does with 150.5 KB):
//   whole   k_route_relax<true>: ONE launch, one workgroup per frame: seeds and bits from d2, the rounds, g written from LDS.
//   tiled   larger grids: k_route_init (t of the seeds to global memory), then launches of k_route_relax<false> — one workgroup per
//           tile of at most 256 x 256 loads its tile and a border of its neighbours' t, relaxes to LOCAL convergence, writes its tile back
//           if it lowered anything — then k_route_final (the pull).  No workgroup waits for another: what crosses tiles crosses launches.
//           A launch in which no tile lowered anything means every tile is converged against its neighbours' final values: the fixed
//           point.  Launches go out in batches; each sets a word when it lowered something, the NEXT launch reads its predecessor's word
//           and leaves at once when that is 0, the host reads the words after the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "nav_tail.h"
#include "plan_handle.h"
#include "../../include/jn_route.h"

namespace jnav {
namespace {

constexpr uint32_t kUnr = JN_ROUTE_UNREACHED;
constexpr int kRtThreads = 512;                     // >= the longest side: one thread per row, then one per column
constexpr int kRtTile = 256;                        // the longest side of a tile of the tiled form
constexpr size_t kRtLdsMax = 160 * 1024;            // one CU's LDS (gfx950)
constexpr int kRtBatchMax = 32;                     // launches of the tiled form between two looks at their words

struct RtArgs {
  int cx, cy, r2, nr2, pen, gr2;
  int tw, th;                                       // the tile (the whole form: the grid)
};
struct RtGoals { int32_t cell[JN_PLAN_MAX_BATCH]; };  // gy * cx + gx per frame (by value: no copy ahead of the launch)
struct RtSlot { uint32_t changed, rounds; };        // one per launch of a batch

// LDS of a w x h rectangle: t with its border, the two bit planes, three words (two round flags, the seed count)
__host__ __device__ inline int rt_pitch(int w) { return 2 * (((w + 3) / 2) | 1); }            // u16 units: an odd number of dwords >= w + 2
__host__ __device__ inline int rt_wpr(int w) { return ((w + 31) / 32) | 1; }                 // words per row of a bit plane, odd
inline size_t rt_lds_bytes(int w, int h) { return (size_t)(h + 2) * rt_pitch(w) * 2 + 2 * (size_t)h * rt_wpr(w) * 4 + 16; }
inline bool rt_whole_fits(int cx, int cy) { return cx <= kRtThreads && cy <= kRtThreads && rt_lds_bytes(cx, cy) <= kRtLdsMax; }

// One sweep of one line: ROW — the cells (k, line), else (line, k); FWD — k rising.  p walks the line in T; the three cells of the next
// column are read before this column's cell is relaxed, the previous column's are in registers (b of it as just written).
template <bool ROW, bool FWD>
DEV bool rt_sweep(uint16_t* T, const uint32_t* __restrict__ P, const uint32_t* __restrict__ N, int pitch, int wpr, int line, int len, int pen) {
  const int step = (ROW ? 1 : pitch) * (FWD ? 1 : -1), side = ROW ? pitch : 1;
  const int k0 = FWD ? 0 : len - 1;
  int p = ROW ? (line + 1) * pitch + k0 + 1 : (k0 + 1) * pitch + line + 1;
  uint32_t am = T[p - step - side], bm = T[p - step], cm = T[p - step + side];
  uint32_t a0 = T[p - side], b0 = T[p], c0 = T[p + side];
  bool ch = false;
  for (int i = 0; i < len; i++, p += step) {
    const uint32_t ap = T[p + step - side], bp = T[p + step], cp = T[p + step + side];
    const int k = FWD ? i : len - 1 - i;
    const int x = ROW ? k : line, y = ROW ? line : k;
    const int wi = y * wpr + (x >> 5);
    const bool pass = (P[wi] >> (x & 31)) & 1u, near = (N[wi] >> (x & 31)) & 1u;
    const uint32_t cand = min(min(min(bm, bp), min(a0, c0)) + 5u, min(min(am, cm), min(ap, cp)) + 7u) + (near ? (uint32_t)pen : 0u);
    if (pass && cand < b0) {                        // b0 <= 65535, so what is stored is <= 65534; a seed's pen is below every cand
      b0 = cand;
      T[p] = (uint16_t)cand;
      ch = true;
    }
    am = a0; bm = b0; cm = c0;
    a0 = ap; b0 = bp; c0 = cp;
  }
  return ch;
}

// WHOLE: gridDim = (n): the frame's grid is the rectangle; out = g.  Else gridDim = (tiles_x, tiles_y, n): tg = t [n][cy][cx] in global
// memory, slots [launch - 1] is read (launch > 0) and slots [launch] written.  Dynamic LDS: rt_lds_bytes(a.tw, a.th).
template <bool WHOLE>
__global__ void __launch_bounds__(kRtThreads) k_route_relax(RtArgs a, RtGoals goals, const uint16_t* __restrict__ d2, uint16_t* tg,
                                                            uint16_t* __restrict__ out, int32_t* __restrict__ seeds, int32_t* __restrict__ rounds,
                                                            RtSlot* slots, int launch) {
  extern __shared__ uint32_t rt_lds[];
  if (!WHOLE && launch > 0 && slots[launch - 1].changed == 0u) return;             // the launch before lowered nothing: converged
  const int frame = WHOLE ? blockIdx.x : blockIdx.z;
  const int x0 = WHOLE ? 0 : blockIdx.x * a.tw, y0 = WHOLE ? 0 : blockIdx.y * a.th;
  const int w = min(a.tw, a.cx - x0), h = min(a.th, a.cy - y0);
  const int pitch = rt_pitch(a.tw), wpr = rt_wpr(a.tw);
  uint16_t* T = reinterpret_cast<uint16_t*>(rt_lds);
  uint32_t* P = rt_lds + (size_t)(a.th + 2) * pitch / 2;
  uint32_t* N = P + (size_t)a.th * wpr;
  uint32_t* flag = N + (size_t)a.th * wpr;                                         // [0], [1]: "this round lowered something"; [2]: seeds
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const size_t fbase = (size_t)frame * a.cx * a.cy;
  const uint16_t* __restrict__ d = d2 + fbase;
  const int goal = goals.cell[frame], gx = goal % a.cx, gy = goal / a.cx;

  if (WHOLE) {
    for (int i = tid; i < (h + 2) * pitch / 2; i += blockDim.x) rt_lds[i] = 0xFFFFFFFFu;
  } else {
    const uint16_t* __restrict__ tf = tg + fbase;
    for (int yy = wave; yy < h + 2; yy += nwaves) {
      const int Y = y0 + yy - 1;
      for (int xx = lane; xx < w + 2; xx += 64) {
        const int X = x0 + xx - 1;
        T[yy * pitch + xx] = (X >= 0 && X < a.cx && Y >= 0 && Y < a.cy) ? tf[(size_t)Y * a.cx + X] : (uint16_t)kUnr;
      }
    }
  }
  if (tid < 3) flag[tid] = 0u;
  __syncthreads();

  // the bit planes, 64 cells of a row per wave step; the whole form seeds t here
  for (int y = wave; y < h; y += nwaves) {
    for (int xc = 0; xc < w; xc += 64) {
      const int x = xc + lane;
      const bool in = x < w;
      const uint32_t v = in ? d[(size_t)(y0 + y) * a.cx + x0 + x] : 0u;
      const bool pass = in && v > (uint32_t)a.r2, near = pass && v <= (uint32_t)a.nr2;
      const unsigned long long pm = __ballot(pass), nm = __ballot(near);
      if (lane == 0) {
        const int wi = y * wpr + (xc >> 5);
        P[wi] = (uint32_t)pm; N[wi] = (uint32_t)nm;
        if ((xc >> 5) + 1 < wpr) { P[wi + 1] = (uint32_t)(pm >> 32); N[wi + 1] = (uint32_t)(nm >> 32); }
      }
      if (WHOLE) {
        const int ex = x - gx, ey = y - gy;
        const bool seed = pass && ex * ex + ey * ey <= a.gr2;
        if (seed) T[(y + 1) * pitch + x + 1] = (uint16_t)(near ? a.pen : 0);
        const unsigned long long sm = __ballot(seed);
        if (lane == 0 && sm) atomicAdd(&flag[2], (uint32_t)__popcll(sm));
      }
    }
  }
  __syncthreads();

  int round = 0;
  for (;;) {
    bool ch = false;
    if (tid < h) {
      ch |= rt_sweep<true, true>(T, P, N, pitch, wpr, tid, w, a.pen);
      ch |= rt_sweep<true, false>(T, P, N, pitch, wpr, tid, w, a.pen);
    }
    __syncthreads();
    if (tid < w) {
      ch |= rt_sweep<false, true>(T, P, N, pitch, wpr, tid, h, a.pen);
      ch |= rt_sweep<false, false>(T, P, N, pitch, wpr, tid, h, a.pen);
    }
    if (ch) flag[round & 1] = 1u;
    if (tid == 0) flag[(round + 1) & 1] = 0u;                                      // last read a round ago, ahead of that round's barrier
    __syncthreads();
    const uint32_t any = __builtin_amdgcn_readfirstlane(flag[round & 1]);          // the same word in every lane: the loop stays scalar
    round++;
    if (!any) break;
  }

  if (WHOLE) {
    // g(c) = the minimum of w + t(m) over the neighbours: jn_route.h's formula on the settled t
    uint16_t* __restrict__ o = out + fbase;
    for (int y = wave; y < h; y += nwaves) {
      for (int x = lane; x < w; x += 64) {
        const int p = (y + 1) * pitch + x + 1;
        const bool pass = (P[y * wpr + (x >> 5)] >> (x & 31)) & 1u;
        const int ex = x - gx, ey = y - gy;
        const uint32_t ax = min(min((uint32_t)T[p - 1], (uint32_t)T[p + 1]), min((uint32_t)T[p - pitch], (uint32_t)T[p + pitch])) + 5u;
        const uint32_t dg = min(min((uint32_t)T[p - pitch - 1], (uint32_t)T[p - pitch + 1]), min((uint32_t)T[p + pitch - 1], (uint32_t)T[p + pitch + 1])) + 7u;
        uint32_t g = min(ax, dg);
        if (g > 65534u) g = kUnr;
        if (ex * ex + ey * ey <= a.gr2) g = 0u;
        o[(size_t)y * a.cx + x] = (uint16_t)(pass ? g : kUnr);
      }
    }
    if (tid == 0) { seeds[frame] = (int32_t)flag[2]; rounds[frame] = round; }
  } else if (round > 1) {                                                          // the first round lowered something
    uint16_t* tf = tg + fbase;
    for (int y = wave; y < h; y += nwaves)
      for (int x = lane; x < w; x += 64) tf[(size_t)(y0 + y) * a.cx + x0 + x] = T[(y + 1) * pitch + x + 1];
    if (tid == 0) {
      slots[launch].changed = 1u;
      atomicMax(&slots[launch].rounds, (uint32_t)round);
    }
  }
}

// the tiled form's first and last kernels, one thread per cell: gridDim = (ceil(cells / 256), n)
__global__ void __launch_bounds__(256) k_route_init(RtArgs a, RtGoals goals, const uint16_t* __restrict__ d2, uint16_t* __restrict__ tg,
                                                    int32_t* __restrict__ seeds) {
  const int cells = a.cx * a.cy, c = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
  bool seed = false;
  if (c < cells) {
    const uint32_t v = d2[(size_t)frame * cells + c];
    const int goal = goals.cell[frame], ex = c % a.cx - goal % a.cx, ey = c / a.cx - goal / a.cx;
    seed = v > (uint32_t)a.r2 && ex * ex + ey * ey <= a.gr2;
    tg[(size_t)frame * cells + c] = (uint16_t)(seed ? (v <= (uint32_t)a.nr2 ? a.pen : 0) : kUnr);
  }
  const unsigned long long sm = __ballot(seed);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(&seeds[frame], (int32_t)__popcll(sm));
}

__global__ void __launch_bounds__(256) k_route_final(RtArgs a, RtGoals goals, const uint16_t* __restrict__ d2, const uint16_t* __restrict__ tg,
                                                     uint16_t* __restrict__ out) {
  const int cells = a.cx * a.cy, c = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
  if (c >= cells) return;
  const int x = c % a.cx, y = c / a.cx;
  const uint16_t* __restrict__ t = tg + (size_t)frame * cells;
  uint32_t ax = kUnr, dg = kUnr;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      if ((dx == 0 && dy == 0) || x + dx < 0 || x + dx >= a.cx || y + dy < 0 || y + dy >= a.cy) continue;
      const uint32_t v = t[(y + dy) * a.cx + x + dx];
      if (dx == 0 || dy == 0) ax = min(ax, v); else dg = min(dg, v);
    }
  uint32_t g = min(ax + 5u, dg + 7u);
  if (g > 65534u) g = kUnr;
  const int goal = goals.cell[frame], ex = x - goal % a.cx, ey = y - goal / a.cx;
  if (ex * ex + ey * ey <= a.gr2) g = 0u;
  out[(size_t)frame * cells + c] = (uint16_t)(d2[(size_t)frame * cells + c] > (uint32_t)a.r2 ? g : kUnr);
}

// rec [n][K], g [n][cells] -> togo [n][K].  gridDim = (ceil(K / 256), n).
__global__ void __launch_bounds__(256) k_route_gather(int K, int cells, const jn_plan_record* __restrict__ rec, const uint16_t* __restrict__ g,
                                                      uint16_t* __restrict__ togo) {
  const int k = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
  if (k >= K) return;
  const int last = rec[(size_t)frame * K + k].last_cell;
  togo[(size_t)frame * K + k] = last < 0 ? (uint16_t)kUnr : g[(size_t)frame * cells + last];
}

bool rt_params_valid(const jn_route_params* rp) {
  return rp && rp->near_radius >= 0 && rp->near_radius <= JN_ROUTE_MAX_NEAR_RADIUS && rp->near_penalty >= 0 &&
         rp->near_penalty <= JN_ROUTE_MAX_NEAR_PENALTY && rp->goal_radius >= 0 && rp->goal_radius <= JN_ROUTE_MAX_GOAL_RADIUS && rp->reserved == 0;
}
bool rt_grid_valid(int cx, int cy, int r2) {
  return cx >= 1 && cx <= JN_COSTMAP_MAX_CELLS && cy >= 1 && cy <= JN_COSTMAP_MAX_CELLS && r2 >= 0 && r2 <= JN_ROUTE_MAX_R2;
}

// jn_route.h "choice" of one frame
void rt_choose(const jn_plan_params& p, double res, const jn_plan_record* rec, const uint16_t* togo, jn_plan_cmd* out) {
  const int K = p.n_v * p.n_w, T = p.steps;
  double best = 0.;
  *out = jn_plan_cmd{0., 0., -1, JN_PLAN_BLOCKED};
  for (int k = 0; k < K; k++) {
    const jn_plan_record& r = rec[k];
    if (r.t_hit != T || r.t_end < 1 || r.t_end > T || togo[k] == kUnr) continue;
    double v, w;
    pl_candidate(p, k, v, w);
    const double dist = ((double)togo[k] * res) / 5.0;
    const double clear = std::min(std::sqrt((double)r.min_d2) * res, p.clear_cap);
    const double score = (p.w_goal * dist - p.w_clear * clear) - p.w_speed * v;
    if (out->candidate < 0 || score < best) {
      best = score;
      *out = jn_plan_cmd{v, w, k, JN_PLAN_OK};
    }
  }
}

// rollout, gather and both copies of n frames into h->h_rec and h->h_togo
jn_status rt_evaluate(jn_plan* h, int n, const uint16_t* dD2, const uint16_t* dTogo, const double* origin, const jn_pose2d* poses) {
  HIP_TRY(hipSetDevice(h->device));
  if (!h->d_togo) {
    const size_t count = (size_t)h->max_batch * h->K;
    if (h->own.alloc(&h->d_togo, count) != hipSuccess || h->own.pinned(&h->h_togo, count) != hipSuccess) {
      h->d_togo = nullptr;                          // whatever was made stays with the owner until the handle goes
      return JN_ERR_NO_DEVICE;
    }
  }
  const jn_status e = pl_enqueue(h, n, dD2, origin, poses);
  if (e != JN_OK) return e;
  hipLaunchKernelGGL(k_route_gather, dim3((unsigned)((h->K + 255) / 256), (unsigned)n), dim3(256), 0, nullptr, h->K, h->cx * h->cy, h->d_rec, dTogo,
                     h->d_togo);
  HIP_TRY(hipMemcpyAsync(h->h_togo, h->d_togo, sizeof(uint16_t) * (size_t)n * h->K, hipMemcpyDeviceToHost, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // namespace
}  // namespace jnav

using namespace jnav;

extern "C" {

void jn_route_params_default(jn_route_params* rp) {
  rp->near_radius = 10; rp->near_penalty = 3; rp->goal_radius = 2; rp->reserved = 0;   // untuned guesses (jn_route.h)
}

jn_status jn_route_goal_cell(double resolution, int32_t cells_x, int32_t cells_y, const double* origin, const double* goal, int32_t* cell) {
  if (!origin || !goal || !cell || !pl_pos(resolution) || !rt_grid_valid(cells_x, cells_y, 0) || !std::isfinite(origin[0]) ||
      !std::isfinite(origin[1]) || !std::isfinite(goal[0]) || !std::isfinite(goal[1]))
    return JN_ERR_INVALID;
  const double fx = std::floor((goal[0] - origin[0]) / resolution), fy = std::floor((goal[1] - origin[1]) / resolution);
  // the clamp in double: the quotient may be infinite or beyond int
  cell[0] = fx >= (double)(cells_x - 1) ? cells_x - 1 : fx >= 0. ? (int32_t)fx : 0;
  cell[1] = fy >= (double)(cells_y - 1) ? cells_y - 1 : fy >= 0. ? (int32_t)fy : 0;
  return JN_OK;
}

jn_status jn_route_field(int32_t device, int32_t n, const uint16_t* dD2, int32_t cells_x, int32_t cells_y, int32_t r2,
                         const jn_route_params* rp, const int32_t* goal_cells, uint16_t* dTogo, int32_t* seeds, jn_route_stats* stats) {
  if (!dD2 || !goal_cells || !dTogo || !seeds || !rt_params_valid(rp) || n < 1 || n > JN_PLAN_MAX_BATCH || !rt_grid_valid(cells_x, cells_y, r2))
    return JN_ERR_INVALID;
  RtGoals goals;
  for (int f = 0; f < n; f++) {
    const int gx = goal_cells[2 * f], gy = goal_cells[2 * f + 1];
    if (gx < 0 || gx >= cells_x || gy < 0 || gy >= cells_y) return JN_ERR_INVALID;
    goals.cell[f] = gy * cells_x + gx;
  }
  for (int f = n; f < JN_PLAN_MAX_BATCH; f++) goals.cell[f] = 0;
  HIP_TRY(hipSetDevice(device));
  RtArgs a;
  a.cx = cells_x; a.cy = cells_y; a.r2 = r2; a.nr2 = rp->near_radius * rp->near_radius; a.pen = rp->near_penalty;
  a.gr2 = rp->goal_radius * rp->goal_radius;
  const size_t cells = (size_t)cells_x * cells_y;
  const bool whole = rt_whole_fits(cells_x, cells_y);
  // scratch: seeds [n] and rounds [n] (int32), the slots of a batch, then the tiled form's t [n][cells]
  const size_t head = ((sizeof(int32_t) * 2 * (size_t)n + sizeof(RtSlot) * kRtBatchMax + 255) / 256) * 256;
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, head + (whole ? 0 : cells * n * sizeof(uint16_t)), &scratch));
  int32_t* dSeeds = static_cast<int32_t*>(scratch);
  int32_t* dRounds = dSeeds + n;
  RtSlot* dSlots = reinterpret_cast<RtSlot*>(dRounds + n);
  uint16_t* dT = reinterpret_cast<uint16_t*>(static_cast<char*>(scratch) + head);
  jn_route_stats st = {whole ? JN_ROUTE_FORM_WHOLE : JN_ROUTE_FORM_TILED, 0, 0, 0};
  int32_t host[2 * JN_PLAN_MAX_BATCH];

  if (whole) {
    a.tw = cells_x; a.th = cells_y;
    const size_t lds = rt_lds_bytes(a.tw, a.th);
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_route_relax<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int threads = std::max(64, ((std::max(cells_x, cells_y) + 63) / 64) * 64);
    hipLaunchKernelGGL(k_route_relax<true>, dim3((unsigned)n), dim3((unsigned)threads), lds, nullptr, a, goals, dD2, (uint16_t*)nullptr, dTogo, dSeeds, dRounds,
                       (RtSlot*)nullptr, 0);
    HIP_TRY(hipMemcpy(host, dSeeds, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipGetLastError());
    st.launches = 1;
    for (int f = 0; f < n; f++) st.rounds = std::max(st.rounds, host[n + f]);
  } else {
    const int tiles_x = (cells_x + kRtTile - 1) / kRtTile, tiles_y = (cells_y + kRtTile - 1) / kRtTile;
    a.tw = (cells_x + tiles_x - 1) / tiles_x; a.th = (cells_y + tiles_y - 1) / tiles_y;
    const size_t lds = rt_lds_bytes(a.tw, a.th);
    if (lds > 64 * 1024)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_route_relax<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int threads = std::max(64, ((std::max(a.tw, a.th) + 63) / 64) * 64);
    const dim3 per_cell((unsigned)((cells + 255) / 256), (unsigned)n);
    HIP_TRY(hipMemsetAsync(dSeeds, 0, sizeof(int32_t) * (size_t)n, nullptr));
    hipLaunchKernelGGL(k_route_init, per_cell, dim3(256), 0, nullptr, a, goals, dD2, dT, dSeeds);
    // every launch that lowers something settles at least one more cell of some frame
    const size_t bound = cells * n + 2;
    size_t launches = 0;
    RtSlot slots[kRtBatchMax];
    bool done = false;
    for (int batch = 4; !done; batch = std::min(2 * batch, kRtBatchMax)) {
      if (launches > bound) return JN_ERR_INTERNAL;
      HIP_TRY(hipMemsetAsync(dSlots, 0, sizeof(RtSlot) * batch, nullptr));
      for (int j = 0; j < batch; j++)
        hipLaunchKernelGGL(k_route_relax<false>, dim3((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n), dim3((unsigned)threads), lds, nullptr, a, goals, dD2,
                           dT, (uint16_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, dSlots, j);
      HIP_TRY(hipMemcpy(slots, dSlots, sizeof(RtSlot) * batch, hipMemcpyDeviceToHost));
      HIP_TRY(hipGetLastError());
      for (int j = 0; j < batch && !done; j++) {
        launches++;                                 // this one ran (its predecessor lowered something, or it is the batch's first)
        st.rounds += (int32_t)std::max(slots[j].rounds, 1u);
        done = slots[j].changed == 0u;
      }
    }
    st.launches = (int32_t)launches;
    hipLaunchKernelGGL(k_route_final, per_cell, dim3(256), 0, nullptr, a, goals, dD2, dT, dTogo);
    HIP_TRY(hipMemcpy(host, dSeeds, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    HIP_TRY(hipGetLastError());
  }
  memcpy(seeds, host, sizeof(int32_t) * (size_t)n);
  if (stats) *stats = st;
  return JN_OK;
}

jn_status jn_route_evaluate(jn_plan* h, int32_t n, const uint16_t* dD2, const uint16_t* dTogo, const double* origin, const jn_pose2d* poses,
                            jn_plan_record* records, uint16_t* togo) {
  if (!pl_call_valid(h, n, dD2, origin, poses) || !dTogo || !records || !togo) return JN_ERR_INVALID;
  const jn_status e = rt_evaluate(h, n, dD2, dTogo, origin, poses);
  if (e != JN_OK) return e;
  memcpy(records, h->h_rec, sizeof(jn_plan_record) * (size_t)n * h->K);
  memcpy(togo, h->h_togo, sizeof(uint16_t) * (size_t)n * h->K);
  return JN_OK;
}

jn_status jn_route_choose(const jn_plan_params* p, double resolution, const jn_plan_record* records, const uint16_t* togo, jn_plan_cmd* out) {
  if (!pl_params_valid(p) || !pl_resolution_valid(p, resolution) || !records || !togo || !out) return JN_ERR_INVALID;
  rt_choose(*p, resolution, records, togo, out);
  return JN_OK;
}

jn_status jn_route_command(jn_plan* h, int32_t n, const uint16_t* dD2, const uint16_t* dTogo, const double* origin, const jn_pose2d* poses,
                           jn_plan_cmd* cmds, jn_plan_record* records, uint16_t* togo) {
  if (!pl_call_valid(h, n, dD2, origin, poses) || !dTogo || !cmds) return JN_ERR_INVALID;
  const jn_status e = rt_evaluate(h, n, dD2, dTogo, origin, poses);
  if (e != JN_OK) return e;
  for (int f = 0; f < n; f++) rt_choose(h->p, h->res, h->h_rec + (size_t)f * h->K, h->h_togo + (size_t)f * h->K, cmds + f);
  if (records) memcpy(records, h->h_rec, sizeof(jn_plan_record) * (size_t)n * h->K);
  if (togo) memcpy(togo, h->h_togo, sizeof(uint16_t) * (size_t)n * h->K);
  return JN_OK;
}

jn_status jn_route_trace(const uint16_t* g, const uint16_t* d2, int32_t cells_x, int32_t cells_y, int32_t r2, const jn_route_params* rp,
                         int32_t start_x, int32_t start_y, int32_t* cells, int32_t capacity, int32_t* length, int32_t* status) {
  if (length) *length = 0;
  if (!g || !d2 || !cells || !length || !status || !rt_params_valid(rp) || !rt_grid_valid(cells_x, cells_y, r2) || capacity < 0) return JN_ERR_INVALID;
  *status = JN_ROUTE_NO_ROUTE;
  if (start_x < 0 || start_x >= cells_x || start_y < 0 || start_y >= cells_y || g[start_y * cells_x + start_x] == kUnr) return JN_OK;
  static const int kDx[8] = {1, -1, 0, 0, 1, -1, 1, -1}, kDy[8] = {0, 0, 1, -1, 1, 1, -1, -1};
  const int nr2 = rp->near_radius * rp->near_radius;
  int x = start_x, y = start_y, len = 0;
  for (;;) {
    if (len >= capacity) return JN_ERR_INVALID;
    cells[len++] = y * cells_x + x;
    const int here = g[y * cells_x + x];
    if (here == 0) break;
    int k = 0;
    for (; k < 8; k++) {
      const int mx = x + kDx[k], my = y + kDy[k];
      if (mx < 0 || mx >= cells_x || my < 0 || my >= cells_y) continue;
      const int m = my * cells_x + mx;
      if ((int)d2[m] <= r2 || g[m] == kUnr) continue;
      if ((k < 4 ? 5 : 7) + ((int)d2[m] <= nr2 ? rp->near_penalty : 0) + (int)g[m] == here) { x = mx; y = my; break; }
    }
    if (k == 8) return JN_ERR_INVALID;              // not the field of these inputs
  }
  *length = len;
  *status = JN_ROUTE_OK;
  return JN_OK;
}

}  // extern "C"

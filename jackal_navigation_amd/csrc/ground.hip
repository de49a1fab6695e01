// ground.hip — the ground-plane estimator (include/jn_ground.h): its kernels, launchers, the host solve and the C entry points.  Product code.
//
// No reference counterpart; the definition is in jn_ground.h, its scalar restatement (the checker) in tests/ground_def.py.  Everything the
// device computes is integer arithmetic, so the bar for scores, hypotheses, winner and sums is bit-identity.
//
// Shape of the two passes over the region (k_ground_score, k_ground_refit): a wave takes a run of up to 256 * NCH pixels of ONE row, each
// lane NCH chunks of four neighbouring pixels (one dwordx4 / dwordx2 load each, in the map's native format), converted to q once and kept
// in registers.  The row is wave-uniform, so of  A x + B y + C q + E  the part  B y + E  is scalar arithmetic, and the inlier test
// |r| <= T is folded into one unsigned compare:  (u64)(r + T) <= 2 T.  k_ground_score then walks the K hypotheses in a wave-uniform loop,
// the hypothesis read by scalar loads from the table k_ground_sample wrote; one evaluation is a v_mad_i64_i32 and a v_cmp_le_u64, the
// count a ballot's s_bcnt1 into a scalar.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstring>
#include <vector>
#include "nav_tail.h"

namespace jnav {
namespace {

// One hypothesis as the scoring passes read it (32 bytes: one s_load_dwordx8).  The test is  (u64)(A x + C q + B y + ept) <= t2  with
// ept = E + T, t2 = 2 T, T = tol_q |C|.  VOID: A = B = C = 0, ept = 1, t2 = 0 — never true.
struct GrHyp {
  int32_t A, B, C, pad;
  int64_t ept, t2;
};

struct GrDev {
  int W, H, x0, y0, x1, y1, K, minq;
  uint32_t seed;
  int tol;
  long long bq, aq;          // the gate's limits in Q16
  long long total;           // n * H * W
  int segs;                  // runs per row
};

DEV uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// ---- sampling: one thread per (frame, hypothesis) ----
template <int FMT>
__global__ void __launch_bounds__(256) k_ground_sample(GrDev s, int n, const typename DispElem<FMT>::T* __restrict__ disp, GrHyp* __restrict__ tab,
                                                        long long* __restrict__ hyps) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * s.K) return;
  const int f = t / s.K, k = t - f * s.K;
  const int rw = s.x1 - s.x0, rh = s.y1 - s.y0;
  int px[3], py[3], pq[3];
  bool ok = true;
  for (int j = 0; j < 3 && ok; j++) {
    bool found = false;
    for (int a = 0; a < 8 && !found; a++) {
      const uint32_t h = mix32(s.seed ^ mix32(((((uint32_t)f * 1024u + (uint32_t)k) * 3u + (uint32_t)j) * 8u) + (uint32_t)a));
      const int x = s.x0 + (int)(((h & 0xffffu) * (uint32_t)rw) >> 16), y = s.y0 + (int)(((h >> 16) * (uint32_t)rh) >> 16);
      int q;
      if (disp_to_q<FMT>(disp[((long long)f * s.H + y) * s.W + x], s.minq, q)) { px[j] = x; py[j] = y; pq[j] = q; found = true; }
    }
    ok = found;
  }
  GrHyp hy = {0, 0, 0, 0, 1, 0};
  long long o[4] = {0, 0, 0, 0};
  if (ok) {
    const long long dx1 = px[1] - px[0], dy1 = py[1] - py[0], dq1 = pq[1] - pq[0];
    const long long dx2 = px[2] - px[0], dy2 = py[2] - py[0], dq2 = pq[2] - pq[0];
    const long long A = dy1 * dq2 - dq1 * dy2, B = dq1 * dx2 - dx1 * dq2, C = dx1 * dy2 - dy1 * dx2;
    const long long aC = C < 0 ? -C : C, aA = A < 0 ? -A : A;
    if (C != 0 && (C > 0 ? -B : B) * 65536 >= s.bq * aC && aA * 65536 <= s.aq * aC) {
      const long long E = -(A * px[0] + B * py[0] + C * pq[0]), T = (long long)s.tol * aC;
      hy.A = (int32_t)A; hy.B = (int32_t)B; hy.C = (int32_t)C; hy.ept = E + T; hy.t2 = 2 * T;
      o[0] = A; o[1] = B; o[2] = C; o[3] = E;
    }
  }
  tab[t] = hy;
#pragma unroll
  for (int i = 0; i < 4; i++) hyps[(long long)t * 4 + i] = o[i];
}

// ---- a wave's run of one row: NCH chunks of four pixels per lane ----
template <int FMT, int NCH>
struct Run {
  int q[NCH][4];
  bool ok[NCH][4];
  int xb[NCH];               // frame x of each chunk's first pixel (may lie left of the region)
};

// task = row * segs + seg of frame f; y wave-uniform.  Loads are whole aligned chunks of the flat array [n * H * W] when `vec`, so a chunk may
// begin before roi_x0 or before the row; elements outside the region are masked, chunks that miss it are not loaded, and a chunk that would
// cross the end of the array is read element by element.
template <int FMT, int NCH>
DEV void load_run(const GrDev& s, const typename DispElem<FMT>::T* __restrict__ disp, int f, int y, int seg, int lane, int vec, Run<FMT, NCH>& r) {
  typedef typename DispElem<FMT>::T T;
  const long long row = ((long long)f * s.H + y) * s.W;
  const long long first = vec ? ((row + s.x0) & ~3ll) : row + s.x0;
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    const long long g = first + 4ll * (((long long)seg * NCH + c) * 64 + lane);
    const int xb = (int)(g - row);
    r.xb[c] = xb;
    T v[4] = {0, 0, 0, 0};
    const bool touches = xb + 3 >= s.x0 && xb < s.x1;
    if (touches) {
      if (vec && g + 3 < s.total) {
        if (sizeof(T) == 4) {
          const float4 w = *reinterpret_cast<const float4*>(disp + g);
          v[0] = (T)w.x; v[1] = (T)w.y; v[2] = (T)w.z; v[3] = (T)w.w;
        } else {
          const short4 w = *reinterpret_cast<const short4*>(disp + g);
          v[0] = (T)w.x; v[1] = (T)w.y; v[2] = (T)w.z; v[3] = (T)w.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (xb + e >= s.x0 && xb + e < s.x1) v[e] = disp[g + e];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
      int q;
      const bool ok = disp_to_q<FMT>(v[e], s.minq, q) && touches && xb + e >= s.x0 && xb + e < s.x1;
      r.q[c][e] = ok ? q : 0;
      r.ok[c][e] = ok;
    }
  }
}

DEV long long mad64(int a, int b, long long c) { return (long long)a * (long long)b + c; }

// Keeps the sign extension of a loop-invariant 32-bit operand inside the loop body: hoisted out of it, instruction selection no longer sees
// sext(a) * sext(b) in one block and emits the four-instruction 64-bit multiply instead of v_mad_i64_i32.  Emits no instruction.
DEV int in_loop(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ---- scoring: the hot path ----
template <int FMT, int NCH>
__global__ void __launch_bounds__(256) k_ground_score(GrDev s, const typename DispElem<FMT>::T* __restrict__ disp, const GrHyp* __restrict__ tab,
                                                       uint32_t* __restrict__ scores, int vec) {
  __shared__ uint32_t cnt[JN_GROUND_MAX_HYPOTHESES];
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int k = threadIdx.x; k < s.K; k += 256) cnt[k] = 0;
  __syncthreads();
  const int tasks = (s.y1 - s.y0) * s.segs;
  const GrHyp* __restrict__ hy = tab + (long long)f * s.K;
  for (int task = blockIdx.x * 4 + wave; task < tasks; task += gridDim.x * 4) {
    const int yr = task / s.segs, seg = task - yr * s.segs, y = s.y0 + yr;
    Run<FMT, NCH> r;
    load_run<FMT, NCH>(s, disp, f, y, seg, lane, vec, r);
    unsigned long long m[NCH][4];
    unsigned long long any = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) { m[c][e] = __ballot(r.ok[c][e]); any |= m[c][e]; }
    if (any == 0) continue;                                    // wave-uniform: nothing valid in this run
    uint32_t acc = 0;
    GrHyp nx = hy[0];                                          // uniform address: scalar loads, one hypothesis ahead
    for (int k = 0; k < s.K; k++) {
      const GrHyp h = nx;
      nx = hy[k + 1 < s.K ? k + 1 : k];
      const long long base = (long long)h.B * y + h.ept;       // scalar
      const unsigned long long t2 = (unsigned long long)h.t2;
      uint32_t c32 = 0;
#pragma unroll
      for (int c = 0; c < NCH; c++) {
        const long long w0 = mad64(h.A, r.xb[c], base);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          const long long u = mad64(h.C, in_loop(r.q[c][e]), w0 + (long long)h.A * e);
          c32 += (uint32_t)__popcll(__ballot((unsigned long long)u <= t2) & m[c][e]);
        }
      }
      acc = lane == (k & 63) ? c32 : acc;                      // lane k % 64 keeps hypothesis k's count
      if ((k & 63) == 63) {
        if (acc) atomicAdd(&cnt[(k & ~63) + lane], acc);
        acc = 0;
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < s.K; k += 256)
    if (cnt[k]) atomicAdd(&scores[(long long)f * s.K + k], cnt[k]);
}

// ---- pick: one wave per frame; the largest count, on a tie the smallest k ----
__global__ void __launch_bounds__(64) k_ground_pick(int K, const uint32_t* __restrict__ scores, int32_t* __restrict__ best) {
  const int f = blockIdx.x, lane = threadIdx.x;
  unsigned long long key = 0;
  for (int k = lane; k < K; k += 64) {
    const unsigned long long v = ((unsigned long long)scores[(long long)f * K + k] << 32) | (uint32_t)(0xffffffffu - (uint32_t)k);
    key = v > key ? v : key;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long v = __shfl_xor(key, o, 64);
    key = v > key ? v : key;
  }
  if (lane == 0) { best[2 * f] = (int32_t)(0xffffffffu - (uint32_t)key); best[2 * f + 1] = (int32_t)(key >> 32); }
}

// ---- refit: the second pass, with the winner; eleven sums per frame ----
template <int FMT, int NCH>
__global__ void __launch_bounds__(256) k_ground_refit(GrDev s, const typename DispElem<FMT>::T* __restrict__ disp, const GrHyp* __restrict__ tab,
                                                       const int32_t* __restrict__ best, unsigned long long* __restrict__ sums, int vec) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tasks = (s.y1 - s.y0) * s.segs;
  const GrHyp h = tab[(long long)f * s.K + best[2 * f]];
  long long a[11];
#pragma unroll
  for (int i = 0; i < 11; i++) a[i] = 0;
  for (int task = blockIdx.x * 4 + wave; task < tasks; task += gridDim.x * 4) {
    const int yr = task / s.segs, seg = task - yr * s.segs, y = s.y0 + yr;
    Run<FMT, NCH> r;
    load_run<FMT, NCH>(s, disp, f, y, seg, lane, vec, r);
    const long long base = (long long)h.B * y + h.ept;
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (!r.ok[c][e]) continue;
        a[10] += 1;
        const long long x = r.xb[c] + e, q = r.q[c][e];
        const long long u = mad64(h.C, r.q[c][e], mad64(h.A, r.xb[c] + e, base));
        if ((unsigned long long)u <= (unsigned long long)h.t2) {
          a[0] += 1; a[1] += x; a[2] += y; a[3] += q;
          a[4] += x * x; a[5] += x * y; a[6] += (long long)y * y; a[7] += x * q; a[8] += y * q; a[9] += q * q;
        }
      }
  }
#pragma unroll
  for (int i = 0; i < 11; i++) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a[i] += __shfl_xor(a[i], o, 64);
    if (lane == 0 && a[i]) atomicAdd(&sums[(long long)f * 11 + i], (unsigned long long)a[i]);
  }
}

// ---------------------------------------------------------------- host ----

// solve M x = b by Gaussian elimination with partial pivoting; false when singular
bool solve4(const double M[16], const double b[4], double x[4]) {
  double a[4][5];
  for (int i = 0; i < 4; i++) { for (int j = 0; j < 4; j++) a[i][j] = M[4 * i + j]; a[i][4] = b[i]; }
  for (int c = 0; c < 4; c++) {
    int p = c;
    for (int i = c + 1; i < 4; i++) if (std::fabs(a[i][c]) > std::fabs(a[p][c])) p = i;
    if (!(std::fabs(a[p][c]) > 0.) || !std::isfinite(a[p][c])) return false;
    if (p != c) for (int j = 0; j < 5; j++) { const double t = a[c][j]; a[c][j] = a[p][j]; a[p][j] = t; }
    for (int i = c + 1; i < 4; i++) {
      const double fct = a[i][c] / a[c][c];
      for (int j = c; j < 5; j++) a[i][j] -= fct * a[c][j];
    }
  }
  for (int i = 3; i >= 0; i--) {
    double v = a[i][4];
    for (int j = i + 1; j < 4; j++) v -= a[i][j] * x[j];
    x[i] = v / a[i][i];
  }
  for (int i = 0; i < 4; i++) if (!std::isfinite(x[i])) return false;
  return true;
}

bool q_transpose_ok(const jn_scan_params* sp, double QT[16]) {
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) QT[4 * i + j] = sp->Q[4 * j + i];
  const double e[4] = {0, 0, 0, 1};
  double x[4];
  return solve4(QT, e, x);
}

bool ground_params_valid(const jn_ground_params* gp, int W, int H) {
  return gp && gp->roi_x0 >= 0 && gp->roi_x0 < gp->roi_x1 && gp->roi_x1 <= W && gp->roi_y0 >= 0 && gp->roi_y0 < gp->roi_y1 && gp->roi_y1 <= H &&
         gp->hypotheses >= 64 && gp->hypotheses <= JN_GROUND_MAX_HYPOTHESES && gp->hypotheses % 64 == 0 && gp->tol_q >= 0 && gp->tol_q <= 65536 &&
         gp->min_disp >= 0 && gp->min_disp <= JN_GROUND_MAX_SIDE && gp->min_inliers >= 0 && gp->reserved == 0 &&
         gp->min_inlier_frac >= 0. && gp->min_inlier_frac <= 1. && std::fabs(gp->beta_min) <= 64. && gp->alpha_max >= 0. && gp->alpha_max <= 64.;
}

double i128_to_double(__int128 v) { return (double)v; }

// the host part of the definition: plane, status, geometry from the sums
void solve_plane(const jn_scan_params* sp, int min_inliers, double min_frac, const int64_t S[10], int64_t valid, jn_ground_plane* o) {
  memcpy(o->sums, S, sizeof(o->sums));
  o->inliers = S[0]; o->valid = valid;
  o->a = o->b = o->c = o->rms = 0.; o->n_cam[0] = o->n_cam[1] = o->n_cam[2] = 0.; o->height_m = 0.;
  o->status = JN_ERR_FEW_SUPPORT;
  const int64_t N = S[0];
  if (N < 3 || N < min_inliers || (double)N < min_frac * (double)valid) return;
  const __int128 n = N, sx = S[1], sy = S[2], sq = S[3];
  const double Mxx = i128_to_double(n * S[4] - sx * sx), Mxy = i128_to_double(n * S[5] - sx * sy), Myy = i128_to_double(n * S[6] - sy * sy);
  const double Mxq = i128_to_double(n * S[7] - sx * sq), Myq = i128_to_double(n * S[8] - sy * sq), Mqq = i128_to_double(n * S[9] - sq * sq);
  const double det = Mxx * Myy - Mxy * Mxy;
  if (!(det > 0.)) return;
  const double aq = (Mxq * Myy - Myq * Mxy) / det, bq = (Myq * Mxx - Mxq * Mxy) / det;
  const double cq = ((double)S[3] - aq * (double)S[1] - bq * (double)S[2]) / (double)N;
  const double sse = Mqq - aq * Mxq - bq * Myq;
  const double a = aq / 16., b = bq / 16., c = cq / 16.;
  double QT[16];
  for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) QT[4 * i + j] = sp->Q[4 * j + i];
  const double pd[4] = {a, b, -1., c - a * sp->crop_offset_x - b * sp->crop_offset_y};
  double p3[4];
  if (!solve4(QT, pd, p3)) return;
  const double len = std::sqrt(p3[0] * p3[0] + p3[1] * p3[1] + p3[2] * p3[2]);
  if (!(len > 0.) || !std::isfinite(len) || p3[3] == 0.) return;
  const double sgn = p3[3] > 0. ? 1. / len : -1. / len;
  o->a = a; o->b = b; o->c = c; o->rms = std::sqrt(sse > 0. ? sse : 0.) / (double)N / 16.;
  for (int i = 0; i < 3; i++) o->n_cam[i] = p3[i] * sgn;
  o->height_m = p3[3] * sgn;
  o->status = JN_OK;
}

// blocks per frame: enough workgroups to fill the chip at n = 1, at most ~2048 in all so that a workgroup's K flushes are shared by many rows
int blocks_per_frame(const GrDev& s, int n) {
  const int tasks = (s.y1 - s.y0) * s.segs;
  int per_frame = (tasks + 3) / 4, cap = 2048 / n;
  if (cap < 1) cap = 1;
  return per_frame > cap ? cap : per_frame;
}

template <int FMT, int NCH>
void launch_passes(hipStream_t st, GrDev s, int n, const typename DispElem<FMT>::T* d, int vec, GrHyp* tab, uint32_t* scores, int32_t* best,
                   unsigned long long* sums) {
  const int rw = s.x1 - s.x0;
  s.segs = (rw + 3 + 256 * NCH - 1) / (256 * NCH);            // + 3: a run may begin up to three pixels left of the region
  const dim3 g(blocks_per_frame(s, n), n);
  hipLaunchKernelGGL((k_ground_score<FMT, NCH>), g, dim3(256), 0, st, s, d, tab, scores, vec);
  hipLaunchKernelGGL(k_ground_pick, dim3(n), dim3(64), 0, st, s.K, scores, best);
  hipLaunchKernelGGL((k_ground_refit<FMT, NCH>), g, dim3(256), 0, st, s, d, tab, best, sums, vec);
}

template <int FMT>
hipError_t launch_ground(hipStream_t st, const GrDev& s, int n, const void* disp, GrHyp* tab, long long* hyps, uint32_t* scores, int32_t* best,
                         unsigned long long* sums) {
  typedef typename DispElem<FMT>::T T;
  const T* d = static_cast<const T*>(disp);
  // the clears on the SAME stream, as costmap.hip's
  hipError_t e = hipMemsetAsync(scores, 0, sizeof(uint32_t) * (size_t)n * s.K, st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(sums, 0, sizeof(unsigned long long) * (size_t)n * 11, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_ground_sample<FMT>), dim3((n * s.K + 255) / 256), dim3(256), 0, st, s, n, d, tab, hyps);
  // wide loads need the four-element chunks of the flat array to be naturally aligned
  const int vec = reinterpret_cast<uintptr_t>(disp) % (4 * sizeof(T)) == 0 ? 1 : 0;
  if (s.x1 - s.x0 > 256) launch_passes<FMT, 2>(st, s, n, d, vec, tab, scores, best, sums);
  else launch_passes<FMT, 1>(st, s, n, d, vec, tab, scores, best, sums);
  return hipSuccess;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

void mat3_mul(const double A[9], const double B[9], double C[9]) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

}  // namespace
}  // namespace jnav

using namespace jnav;

extern "C" {

void jn_ground_params_default(jn_ground_params* gp, int32_t W, int32_t H) {
  gp->roi_x0 = 0; gp->roi_x1 = W; gp->roi_y0 = H / 2; gp->roi_y1 = H;
  gp->hypotheses = 256; gp->tol_q = 8; gp->min_disp = 1; gp->min_inliers = 500; gp->seed = 0x9e3779b9u; gp->reserved = 0;
  gp->min_inlier_frac = 0.2; gp->beta_min = 0.02; gp->alpha_max = 0.25;
}

jn_status jn_ground_estimate(int32_t device, const jn_scan_params* sp, const jn_ground_params* gp, int32_t n, const void* dDisp, int32_t format,
                             int32_t W, int32_t H, jn_ground_plane* out, int32_t* scores, int64_t* hyps) {
  double QT[16];
  if (!sp || !gp || !dDisp || !out || n < 1 || W < 1 || H < 1 || W > JN_GROUND_MAX_SIDE || H > JN_GROUND_MAX_SIDE ||
      (format != JN_GROUND_F32 && format != JN_GROUND_I16 && format != JN_GROUND_I16_SUB) || !ground_params_valid(gp, W, H) ||
      n > 65535 || !q_transpose_ok(sp, QT))
    return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  GrDev s;
  s.W = W; s.H = H; s.x0 = gp->roi_x0; s.y0 = gp->roi_y0; s.x1 = gp->roi_x1; s.y1 = gp->roi_y1; s.K = gp->hypotheses; s.minq = 16 * gp->min_disp;
  s.seed = gp->seed; s.tol = gp->tol_q;
  s.bq = llrint(16. * gp->beta_min * 65536.); s.aq = llrint(16. * gp->alpha_max * 65536.);
  s.total = (long long)n * H * W; s.segs = 1;
  const size_t K = (size_t)s.K;
  const size_t o_tab = 0, o_hyps = o_tab + align256(sizeof(GrHyp) * n * K), o_scores = o_hyps + align256(32 * n * K),
               o_best = o_scores + align256(4 * n * K), o_sums = o_best + align256(8 * (size_t)n), need = o_sums + align256(88 * (size_t)n);
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, need, &scratch));
  char* const p = static_cast<char*>(scratch);
  GrHyp* tab = reinterpret_cast<GrHyp*>(p + o_tab);
  long long* dh = reinterpret_cast<long long*>(p + o_hyps);
  uint32_t* dsc = reinterpret_cast<uint32_t*>(p + o_scores);
  int32_t* dbest = reinterpret_cast<int32_t*>(p + o_best);
  unsigned long long* dsums = reinterpret_cast<unsigned long long*>(p + o_sums);
  const hipError_t launched = format == JN_GROUND_F32   ? launch_ground<JN_GROUND_F32>(nullptr, s, n, dDisp, tab, dh, dsc, dbest, dsums)
                             : format == JN_GROUND_I16 ? launch_ground<JN_GROUND_I16>(nullptr, s, n, dDisp, tab, dh, dsc, dbest, dsums)
                                                       : launch_ground<JN_GROUND_I16_SUB>(nullptr, s, n, dDisp, tab, dh, dsc, dbest, dsums);
  HIP_TRY(launched);                                           // (the macro prints its argument: no JN_ names in it, tests/test_abi.py counts them)
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> hb(2 * (size_t)n);
  std::vector<int64_t> hs(11 * (size_t)n);
  HIP_TRY(hipMemcpy(hb.data(), dbest, 8 * (size_t)n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hs.data(), dsums, 88 * (size_t)n, hipMemcpyDeviceToHost));
  if (scores) HIP_TRY(hipMemcpy(scores, dsc, 4 * n * K, hipMemcpyDeviceToHost));
  if (hyps) HIP_TRY(hipMemcpy(hyps, dh, 32 * n * K, hipMemcpyDeviceToHost));
  for (int f = 0; f < n; f++) {
    solve_plane(sp, gp->min_inliers, gp->min_inlier_frac, &hs[11 * (size_t)f], hs[11 * (size_t)f + 10], &out[f]);
    out[f].best = hb[2 * f];
  }
  return JN_OK;
}

jn_status jn_ground_solve(const jn_scan_params* sp, const jn_ground_params* gp, const int64_t sums[10], int64_t valid, jn_ground_plane* out) {
  double QT[16];
  if (!sp || !gp || !sums || !out || !q_transpose_ok(sp, QT) || gp->min_inliers < 0 || !(gp->min_inlier_frac >= 0. && gp->min_inlier_frac <= 1.))
    return JN_ERR_INVALID;
  solve_plane(sp, gp->min_inliers, gp->min_inlier_frac, sums, valid, out);
  out->best = 0;
  return JN_OK;
}

void jn_ground_nominal_prior(double XR[9], double XT[3]) {
  const double R[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0};
  memcpy(XR, R, sizeof R);
  XT[0] = XT[1] = XT[2] = 0.;
}

jn_status jn_ground_align(const double n_cam[3], double height_m, const double XR0[9], const double XT0[3], double max_tilt_deg, double XR[9],
                          double XT[3], double* tilt_deg) {
  if (!n_cam || !XR0 || !XT0 || !XR || !XT || !(height_m > 0.) || !std::isfinite(height_m) || !(max_tilt_deg >= 0.)) return JN_ERR_INVALID;
  for (int i = 0; i < 9; i++) if (!std::isfinite(XR0[i])) return JN_ERR_INVALID;
  const double ln = std::sqrt(n_cam[0] * n_cam[0] + n_cam[1] * n_cam[1] + n_cam[2] * n_cam[2]);
  const double u_raw[3] = {XR0[6], XR0[7], XR0[8]};                      // XR0^T e_z: the third row
  const double lu = std::sqrt(u_raw[0] * u_raw[0] + u_raw[1] * u_raw[1] + u_raw[2] * u_raw[2]);
  if (!(ln > 0.) || !std::isfinite(ln) || !(lu > 0.)) return JN_ERR_INVALID;
  const double nv[3] = {n_cam[0] / ln, n_cam[1] / ln, n_cam[2] / ln}, u[3] = {u_raw[0] / lu, u_raw[1] / lu, u_raw[2] / lu};
  const double ax[3] = {nv[1] * u[2] - nv[2] * u[1], nv[2] * u[0] - nv[0] * u[2], nv[0] * u[1] - nv[1] * u[0]};
  const double sn = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), cs = nv[0] * u[0] + nv[1] * u[1] + nv[2] * u[2];
  const double tilt = std::atan2(sn, cs) * 180. / 3.14159265358979323846;
  double Rd[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (sn < 1e-15) {
    if (cs < 0.) return JN_ERR_INVALID;                                   // antiparallel: no smallest rotation
  } else {
    if (tilt_deg) *tilt_deg = tilt;
    if (tilt > max_tilt_deg) return JN_ERR_INVALID;
    const double k[3] = {ax[0] / sn, ax[1] / sn, ax[2] / sn};
    const double Kx[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
    double K2[9];
    mat3_mul(Kx, Kx, K2);
    for (int i = 0; i < 9; i++) Rd[i] += sn * Kx[i] + (1. - cs) * K2[i];
  }
  if (tilt_deg) *tilt_deg = tilt;
  double out[9];
  mat3_mul(XR0, Rd, out);
  memcpy(XR, out, sizeof out);
  XT[0] = XT0[0]; XT[1] = XT0[1]; XT[2] = height_m;
  return JN_OK;
}

jn_status jn_ground_extrinsics(const jn_ground_plane* planes, int32_t n, const jn_scan_params* sp, double max_tilt_deg, double XR[9], double XT[3],
                               double* tilt_deg) {
  double QT[16];
  if (!planes || n < 1 || !sp || !XR || !XT || !q_transpose_ok(sp, QT)) return JN_ERR_INVALID;
  int64_t S[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, valid = 0;
  int used = 0;
  for (int f = 0; f < n; f++) {
    if (planes[f].status != JN_OK) continue;
    for (int i = 0; i < 10; i++) S[i] += planes[f].sums[i];
    valid += planes[f].valid;
    used++;
  }
  if (!used) return JN_ERR_FEW_SUPPORT;
  jn_ground_plane joint;
  solve_plane(sp, 0, 0., S, valid, &joint);
  if (joint.status != JN_OK) return JN_ERR_FEW_SUPPORT;
  return jn_ground_align(joint.n_cam, joint.height_m, sp->XR, sp->XT, max_tilt_deg, XR, XT, tilt_deg);
}

}  // extern "C"

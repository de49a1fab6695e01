// scan.hip — the node side (point_cloud.cpp) on gfx950: the mono8 conversion, the valid-disparity table, the obstacle scan, the rectification
// front end and the point cloud.  Product code.
//
// What every matcher handle, the costmap, the ROS node and the stateless jn_* entry points call behind a disparity map; none of it is ELAS.
// The reprojection, the ground model and the order-preserving double <-> uint64 map are nav_tail.h's, shared with the navigation tails,
// whose bar is bit-identity with this scan.  Built like kernels.hip (-fhip-fp32-correctly-rounded-divide-sqrt: k_undistort_map / k_remap).
#include "nav_tail.h"

namespace jnav {

// convertTo(CV_8U) (point_cloud.cpp:422) = round-half-even + saturate.
DEV uint8_t f32_to_u8(float x) {
  const float r = rintf(x);
  return (uint8_t)(r < 0.f ? 0 : (r > 255.f ? 255 : (int)r));
}
__global__ void __launch_bounds__(256) k_to_u8(const float* __restrict__ D, uint8_t* __restrict__ out, long long count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = f32_to_u8(D[i]);
}

// cacheDisparityValues (point_cloud.cpp:104-147)
__global__ void __launch_bounds__(256) k_valid_lut(NavGeom s, int W, int H, uint8_t* __restrict__ lut) {
  const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
  if (i >= W) return;
  int d;
  for (d = 3; d <= 255; d++) {
    double X, Y, Z;
    if (!nav_reproject(s, i, j, (double)d, X, Y, Z)) continue;
    if (Z < 0.) continue;
    if (nav_is_ground(s, X, Z)) continue;
    break;
  }
  lut[((size_t)j * W + i) * 2] = (uint8_t)d;       // 256 wraps to 0 like the reference's uchar store (:142)
  lut[((size_t)j * W + i) * 2 + 1] = 255;
}

// publishObstacleScan(Mat&) (point_cloud.cpp:213-296).  Per block: bins and the four extrema are
// reduced in LDS (64-bit integer atomics on order-encoded doubles), then merged into global memory.
// kFromCloud selects the -g flavour (publishPointCloud + publishObstacleScan(vector<Point3d>),
// point_cloud.cpp:321-352, :149-211): every pixel with d >= 2 becomes a point, points on the ground
// model are dropped, the rest are binned — instead of the LUT test of the default path.
constexpr int kScanRows = 16;
// kSgm: the disparities come from the SGM mode's winners (sgm_sweep.hip): the L/R check (k_sw_lr), the int16 map, its mono8 form
// (jn_sgm_disparity_to_u8's rounding) and the scan in ONE pass — the three-kernel tail read the int16 map back twice and the mono8 map once.
// The winners of a thread's 16 rows are requested together (a left winner, then the right image's winner it points at: two dependent
// loads, which one row at a time would pay 16 times).
template <bool kFromCloud, bool kSgm = false>
__global__ void __launch_bounds__(256) k_scan(NavGeom s, const float* __restrict__ dD, uint8_t* __restrict__ dDisp,
                                              const uint8_t* __restrict__ lut, int W, int H, unsigned long long* __restrict__ gbins,
                                              unsigned long long* __restrict__ gmeta, SgmWinners sw = SgmWinners()) {
  extern __shared__ unsigned long long lds[];      // [bins] + 4
  unsigned long long* lbins = lds;
  unsigned long long* lmeta = lds + s.bins;
  const int frame = blockIdx.z;
  for (int k = threadIdx.x; k < s.bins; k += 256) lbins[k] = ~0ull;
  if (threadIdx.x < 4) lmeta[threadIdx.x] = (threadIdx.x & 1) ? 0ull : ~0ull;   // min slots start high, max slots low
  __syncthreads();
  // One thread walks kScanRows rows of one column.  The bearing of a pixel hardly depends on its row or
  // disparity, so consecutive rows fall in the same bin: the running minimum stays in registers and reaches the
  // LDS only when the bin changes (same-address LDS atomics from a whole wave would serialise otherwise).
  const int i = blockIdx.x * 256 + threadIdx.x, j0 = blockIdx.y * kScanRows;
  unsigned long long tmin = ~0ull, tmax = 0ull, rmin = ~0ull, rmax = 0ull;
  int cur_bin = -1;
  unsigned long long cur_min = ~0ull;
  const int jend = min(j0 + kScanRows, H);
  // Phase 1: the inputs of all of the thread's rows are requested TOGETHER (16 independent loads per array; round 4 fetched one row ahead
  // and the kernel ran at one load latency per row), the mono8 map is written, and the rows whose disparity passes the LUT test (or d >= 2
  // for the -g flavour) are noted in a mask.  Phase 2 visits only those rows, in ascending order — the order the running bin minimum expects.
  uint32_t u8pk[kScanRows / 4] = {};                              // the mono8 values of this thread's rows
  uint32_t cand = 0;
  if (i < W) {
    const size_t p0 = ((size_t)frame * H + j0) * W + i;
    int dv[kScanRows];
    if constexpr (kSgm) {
      const int xk = W - 1 - i;                                   // the sweeps work on x-mirrored columns
      uint32_t e[kScanRows], m[kScanRows];
#pragma unroll
      for (int r = 0; r < kScanRows; r++) e[r] = sw.dl[((size_t)frame * H + min(j0 + r, H - 1)) * W + xk];
#pragma unroll
      for (int r = 0; r < kScanRows; r++) m[r] = sw.minr[((size_t)frame * H + min(j0 + r, H - 1)) * W + min(xk + (int)(e[r] & 0xFFFFu), W - 1)];
#pragma unroll
      for (int r = 0; r < kScanRows; r++) {
        const int d = (int)(e[r] & 0xFFFFu);
        const bool ok = sw.lr < 0 || (xk + d < W && abs(d - (int)(m[r] & 0xFFFFu)) <= sw.lr);    // x - d >= 0 and the right image's winner there agrees
        int v = ok ? (sw.subpixel ? (int)(int16_t)(e[r] >> 16) : d) : (sw.subpixel ? -16 : -1);
        if (j0 + r < H) sw.disp[p0 + (size_t)r * W] = (int16_t)v;
        if (v < 0) v = 0;
        else if (sw.subpixel) { const int q = v >> 4, f = v & 15; v = q + ((f > 8 || (f == 8 && (q & 1))) ? 1 : 0); }   // half to even, as jn_sgm_disparity_to_u8
        dv[r] = min(v, 255);
        if (j0 + r < H) dDisp[p0 + (size_t)r * W] = (uint8_t)dv[r];
      }
    } else if (dD) {
      float fd[kScanRows];
#pragma unroll
      for (int r = 0; r < kScanRows; r++) fd[r] = dD[((size_t)frame * H + min(j0 + r, H - 1)) * W + i];
#pragma unroll
      for (int r = 0; r < kScanRows; r++) { dv[r] = f32_to_u8(fd[r]); if (j0 + r < H) dDisp[p0 + (size_t)r * W] = (uint8_t)dv[r]; }
    } else {
#pragma unroll
      for (int r = 0; r < kScanRows; r++) dv[r] = dDisp[((size_t)frame * H + min(j0 + r, H - 1)) * W + i];
    }
    uint32_t lt[kScanRows];
    if (!kFromCloud) {
#pragma unroll
      for (int r = 0; r < kScanRows; r++) lt[r] = reinterpret_cast<const uint16_t*>(lut)[(size_t)min(j0 + r, H - 1) * W + i];       // :234
    }
#pragma unroll
    for (int r = 0; r < kScanRows; r++) {
      u8pk[r >> 2] |= (uint32_t)dv[r] << (8 * (r & 3));
      const bool c = kFromCloud ? dv[r] >= 2 : (dv[r] >= (int)(lt[r] & 0xFF) && dv[r] <= (int)(lt[r] >> 8));
      if (c && j0 + r < jend) cand |= 1u << r;
    }
  }
  for (uint32_t mk = cand; mk; mk &= mk - 1) {
    const int rr = __ffs((int)mk) - 1, j = j0 + rr;
    const uint32_t w = rr < 8 ? (rr < 4 ? u8pk[0] : u8pk[1]) : (rr < 12 ? u8pk[2] : u8pk[3]);
    const int d = (int)((w >> (8 * (rr & 3))) & 255u);
    bool take;
    double X = 0, Y = 0, Z = 0;
    if (kFromCloud) take = nav_reproject(s, i, j, (double)d, X, Y, Z) && !nav_is_ground(s, X, Z);               // :324 (d >= 2: the mask), :166-172
    else take = nav_reproject(s, i, j, (double)d, X, Y, Z);                                                  // (the LUT test: the mask)
    if (take) {
      const double th = atan2(Y, X);
      const double deg = __dmul_rn(th, 180.) / s.pi;
      const double r = sqrt(__dadd_rn(__dmul_rn(Y, Y), __dmul_rn(X, X)));
      const unsigned long long et = nav_enc(th), er = nav_enc(r);
      tmin = min(tmin, et); tmax = max(tmax, et); rmin = min(rmin, er); rmax = max(rmax, er);
      const double kf = floor(__dmul_rn((double)s.bins, __dadd_rn(s.fov / 2., -deg)) / s.fov);   // :263
      if (kf >= 0 && kf < (double)s.bins) {
        const int k = (int)kf;
        if (k != cur_bin) {
          if (cur_bin >= 0) atomicMin(&lbins[cur_bin], cur_min);
          cur_bin = k; cur_min = er;
        } else cur_min = min(cur_min, er);
      }
    }
  }
  if (cur_bin >= 0) atomicMin(&lbins[cur_bin], cur_min);
  // extrema: butterfly inside the wave, then one LDS atomic per wave — skipped by the (many) waves in which
  // no pixel passed the test
  if (__ballot(tmin != ~0ull) != 0ull) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    tmin = min(tmin, __shfl_xor(tmin, off)); tmax = max(tmax, __shfl_xor(tmax, off));
    rmin = min(rmin, __shfl_xor(rmin, off)); rmax = max(rmax, __shfl_xor(rmax, off));
  }
  if ((threadIdx.x & 63) == 0) { atomicMin(&lmeta[0], tmin); atomicMax(&lmeta[1], tmax); atomicMin(&lmeta[2], rmin); atomicMax(&lmeta[3], rmax); }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < s.bins; k += 256)
    if (lbins[k] != ~0ull) atomicMin(&gbins[(size_t)frame * s.bins + k], lbins[k]);
  if (threadIdx.x < 4) {
    const unsigned long long x = lmeta[threadIdx.x];
    if (threadIdx.x & 1) { if (x != 0ull) atomicMax(&gmeta[frame * 4 + threadIdx.x], x); }
    else { if (x != ~0ull) atomicMin(&gmeta[frame * 4 + threadIdx.x], x); }
  }
}
__global__ void k_scan_init(int total_bins, int n, unsigned long long* gbins, unsigned long long* gmeta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total_bins) gbins[i] = ~0ull;
  if (i < n * 4) gmeta[i] = (i & 1) ? 0ull : ~0ull;
}
__global__ void k_scan_finish(int total_bins, int n, unsigned long long* gbins, const unsigned long long* gmeta, double* meta, double* flat) {
  // flat (may be null): the cross-rig merge's packed buffer [bins of all frames | extrema of all frames, maxima negated] — written here
  // so that a batch with a communicator attached needs no separate pack launch (comm.cpp)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total_bins) {
    const unsigned long long k = gbins[i];
    const double x = (k == ~0ull) ? 1e9 : nav_dec(k);                              // INF of point_cloud.cpp:54
    reinterpret_cast<double*>(gbins)[i] = x;
    if (flat) flat[i] = x;
  }
  if (i < n * 4) {
    const unsigned long long k = gmeta[i];
    const double init[4] = {400., -400., 1e9, -500.};                          // point_cloud.cpp:219-220
    const bool untouched = (i & 1) ? (k == 0ull) : (k == ~0ull);
    const double x = untouched ? init[i & 3] : nav_dec(k);
    meta[i] = x;
    if (flat) flat[total_bins + i] = (i & 1) ? -x : x;
  }
}

// Cross-rig merge (comm.cpp): bins [n][bins] and extrema [n][4] of a batch <-> one packed buffer, the two maxima of
// every frame negated (exact for doubles) so that the whole merge is a single MIN all-reduce.
__global__ void k_scan_pack(int nb, int nm, double* __restrict__ bins, double* __restrict__ meta, double* __restrict__ flat, int pack) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nb) { if (pack) flat[i] = bins[i]; else bins[i] = flat[i]; }
  else if (i < nb + nm) {
    const int j = i - nb;
    if (pack) { const double x = meta[j]; flat[i] = (j & 1) ? -x : x; }
    else { const double x = flat[i]; meta[j] = (j & 1) ? -x : x; }
  }
}

// initUndistortRectifyMap (point_cloud.cpp:553-554): for every rectified pixel the distorted source
// position.  iR = inverse(P[:, :3] * R) comes from the host; the per-pixel math is OpenCV's, in
// double, stored as float (the column walk is evaluated directly instead of by repeated addition).
struct MapDev { double iR[9], k1, k2, p1, p2, k3, fx, fy, u0, v0; };
__global__ void __launch_bounds__(256) k_undistort_map(MapDev m, int W, int H, float* __restrict__ mapx, float* __restrict__ mapy) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= W) return;
  const double fj = (double)j, fi = (double)i;
  const double _x = __dadd_rn(__dadd_rn(__dmul_rn(fj, m.iR[0]), __dmul_rn(fi, m.iR[1])), m.iR[2]);
  const double _y = __dadd_rn(__dadd_rn(__dmul_rn(fj, m.iR[3]), __dmul_rn(fi, m.iR[4])), m.iR[5]);
  const double _w = __dadd_rn(__dadd_rn(__dmul_rn(fj, m.iR[6]), __dmul_rn(fi, m.iR[7])), m.iR[8]);
  const double w = __ddiv_rn(1.0, _w), x = __dmul_rn(_x, w), y = __dmul_rn(_y, w);
  const double x2 = __dmul_rn(x, x), y2 = __dmul_rn(y, y), r2 = __dadd_rn(x2, y2), _2xy = __dmul_rn(__dmul_rn(2.0, x), y);
  const double kr = __dadd_rn(1.0, __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(m.k3, r2), m.k2), r2), m.k1), r2));
  const double u = __dadd_rn(__dmul_rn(m.fx, __dadd_rn(__dadd_rn(__dmul_rn(x, kr), __dmul_rn(m.p1, _2xy)),
                                                        __dmul_rn(m.p2, __dadd_rn(r2, __dmul_rn(2.0, x2))))), m.u0);
  const double v = __dadd_rn(__dmul_rn(m.fy, __dadd_rn(__dadd_rn(__dmul_rn(y, kr), __dmul_rn(m.p1, __dadd_rn(r2, __dmul_rn(2.0, y2)))),
                                                        __dmul_rn(m.p2, _2xy))), m.v0);
  mapx[(size_t)i * W + j] = (float)u;
  mapy[(size_t)i * W + j] = (float)v;
}

// remap, INTER_LINEAR, BORDER_CONSTANT 0 (point_cloud.cpp:440, :481)
__global__ void __launch_bounds__(256) k_remap(const uint8_t* __restrict__ src, int sw, int sh, int spitch, long long sstride,
                                               const float* __restrict__ mapx, const float* __restrict__ mapy,
                                               uint8_t* __restrict__ dst, int W, int H, int dpitch, long long dstride) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, img = blockIdx.z;
  if (x >= W) return;
  const float qx = rintf(__fmul_rn(mapx[(size_t)y * W + x], 32.0f)), qy = rintf(__fmul_rn(mapy[(size_t)y * W + x], 32.0f));
  uint8_t* out = dst + (long long)img * dstride + (size_t)y * dpitch + x;
  // NaN (what k_undistort_map writes where _w == 0), or a 1/32-pixel value outside int32: outside every image, the border value.
  // The conversion alone would turn NaN into 0, i.e. into source pixel (0, 0).
  if (!(qx >= -2147483648.0f && qx < 2147483648.0f && qy >= -2147483648.0f && qy < 2147483648.0f)) { *out = 0; return; }
  const int sx = (int)qx, sy = (int)qy;
  const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
  const uint8_t* S = src + (long long)img * sstride;
  auto tap = [&](int xx, int yy) -> int { return (xx >= 0 && xx < sw && yy >= 0 && yy < sh) ? S[(size_t)yy * spitch + xx] : 0; };
  const int p00 = tap(ix, iy), p01 = tap(ix + 1, iy), p10 = tap(ix, iy + 1), p11 = tap(ix + 1, iy + 1);
  const int acc = (32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p01 + (32 - fx) * fy * p10 + fx * fy * p11;
  *out = (uint8_t)((acc + 512) >> 10);
}

// Point cloud (-g, point_cloud.cpp:321-352): column-major order (i outer, j inner) with d >= 2.
__global__ void __launch_bounds__(256) k_pc_count(const uint8_t* __restrict__ disp, int W, int H, long long* __restrict__ col_count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W) return;
  int c = 0;
  for (int j = 0; j < H; j++) c += disp[(size_t)j * W + i] >= 2;
  col_count[i + 1] = c;
  if (i == 0) col_count[0] = 0;
}
__global__ void k_pc_scan(int W, long long* col_count) {   // tiny: one thread, W <= a few thousand
  if (threadIdx.x == 0 && blockIdx.x == 0) for (int i = 1; i <= W; i++) col_count[i] += col_count[i - 1];
}
__global__ void __launch_bounds__(256) k_pc_scatter(NavGeom s, const uint8_t* __restrict__ disp, int W, int H,
                                                    const long long* __restrict__ col_count, float* __restrict__ xyz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= W) return;
  long long o = col_count[i];
  for (int j = 0; j < H; j++) {
    const int d = disp[(size_t)j * W + i];
    if (d < 2) continue;
    double X, Y, Z;
    if (!nav_reproject(s, i, j, (double)d, X, Y, Z)) { X = Y = Z = 0; }
    xyz[3 * o] = (float)X; xyz[3 * o + 1] = (float)Y; xyz[3 * o + 2] = (float)Z; o++;
  }
}

// ================================================================================================
// launchers
void launch_to_u8(hipStream_t st, const float* D, uint8_t* out, int64_t count) {
  hipLaunchKernelGGL(k_to_u8, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, D, out, (long long)count);
}
void launch_valid_lut(hipStream_t st, const jn_scan_params& sp, int W, int H, uint8_t* lut) {
  hipLaunchKernelGGL(k_valid_lut, grid2d(W, H, 1), dim3(256), 0, st, nav_geom(sp), W, H, lut);
}
void launch_scan(hipStream_t st, const jn_scan_params& sp, int n, const float* dD, uint8_t* dDisp, const uint8_t* lut,
                 int W, int H, double* bins, double* meta, unsigned long long* scratch, double* flat, const SgmWinners* sgm) {
  const NavGeom s = nav_geom(sp);
  unsigned long long* gb = reinterpret_cast<unsigned long long*>(bins);
  const int total = n * s.bins, m = total > n * 4 ? total : n * 4;
  hipLaunchKernelGGL(k_scan_init, dim3((m + 255) / 256), dim3(256), 0, st, total, n, gb, scratch);
  const dim3 sg((W + 255) / 256, (H + kScanRows - 1) / kScanRows, n);
  if (sgm) hipLaunchKernelGGL((k_scan<false, true>), sg, dim3(256), (s.bins + 4) * sizeof(unsigned long long), st, s, nullptr, dDisp, lut, W, H, gb, scratch, *sgm);
  else if (lut) hipLaunchKernelGGL((k_scan<false>), sg, dim3(256), (s.bins + 4) * sizeof(unsigned long long), st, s, dD, dDisp, lut, W, H, gb, scratch, SgmWinners());
  else     hipLaunchKernelGGL((k_scan<true>), sg, dim3(256), (s.bins + 4) * sizeof(unsigned long long), st, s, dD, dDisp, lut, W, H, gb, scratch, SgmWinners());
  hipLaunchKernelGGL(k_scan_finish, dim3((m + 255) / 256), dim3(256), 0, st, total, n, gb, scratch, meta, flat);
}
void launch_scan_pack(hipStream_t st, int n, int bins, double* dBins, double* dMeta, double* flat, bool pack) {
  const int nb = n * bins, nm = n * 4;
  hipLaunchKernelGGL(k_scan_pack, dim3((nb + nm + 255) / 256), dim3(256), 0, st, nb, nm, dBins, dMeta, flat, pack ? 1 : 0);
}
void launch_undistort_map(hipStream_t st, const double iR[9], const double K[9], const double D[5], int W, int H, float* mapx, float* mapy) {
  MapDev m;
  for (int i = 0; i < 9; i++) m.iR[i] = iR[i];
  m.k1 = D[0]; m.k2 = D[1]; m.p1 = D[2]; m.p2 = D[3]; m.k3 = D[4];
  m.fx = K[0]; m.fy = K[4]; m.u0 = K[2]; m.v0 = K[5];
  hipLaunchKernelGGL(k_undistort_map, grid2d(W, H, 1), dim3(256), 0, st, m, W, H, mapx, mapy);
}
void launch_remap(hipStream_t st, int n, const uint8_t* src, int sw, int sh, int spitch, int64_t sstride, const float* mapx,
                  const float* mapy, uint8_t* dst, int W, int H, int dpitch, int64_t dstride) {
  hipLaunchKernelGGL(k_remap, grid2d(W, H, n), dim3(256), 0, st, src, sw, sh, spitch, (long long)sstride, mapx, mapy, dst, W, H, dpitch,
                     (long long)dstride);
}
void launch_point_cloud(hipStream_t st, const jn_scan_params& sp, const uint8_t* disp, int W, int H, float* xyz, long long* col_count) {
  const NavGeom s = nav_geom(sp);
  hipLaunchKernelGGL(k_pc_count, dim3((W + 255) / 256), dim3(256), 0, st, disp, W, H, col_count);
  hipLaunchKernelGGL(k_pc_scan, dim3(1), dim3(64), 0, st, W, col_count);
  hipLaunchKernelGGL(k_pc_scatter, dim3((W + 255) / 256), dim3(256), 0, st, s, disp, W, H, col_count, xyz);
}

}  // namespace jnav

// ================================================================================================
// the C entry points of the node side (include/jn_stereo.h: "seam B2" and the rectification front end)
#include <cstring>

using namespace jnav;

extern "C" {

void jn_scan_params_default(jn_scan_params* sp, int32_t W, int32_t H) {
  // K1 / T of calibration/amrl_jackal_webcam_stereo.yml (calibrated at 640x360, point_cloud.cpp:38),
  // scaled to the working size; Q in the zero-disparity form stereoRectify emits.
  const double sx = (double)W / 640.0, sy = (double)H / 360.0;
  const double f = 4.6417933392659904e+02 * sx, cx = 3.2479711799310849e+02 * sx, cy = 1.8685472713963392e+02 * sy;
  const double Tx = -9.4052586442980660e-02;
  const double Q[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 0, f, 0, 0, -1.0 / Tx, 0};
  memcpy(sp->Q, Q, sizeof(Q));
  const double XR[9] = {-0.0007962732853436516, -0.2675000227968607, 0.9635575706420958,
                        -0.9999984502796089, -0.001321509725770019, -0.00119326128710218,
                        0.001592547981999815, -0.9635569909380592, -0.2674985457970802};
  memcpy(sp->XR, XR, sizeof(XR));
  sp->XT[0] = 0; sp->XT[1] = 0; sp->XT[2] = 0.28;
  sp->crop_offset_x = 0; sp->crop_offset_y = 0;
  sp->gp_height_thresh = 0.05; sp->gp_angle_thresh = 4. * 3.1415 / 180.; sp->gp_dist_thresh = 1.0;
  sp->fov_deg = 90.; sp->bins = 90; sp->pi_approx = 3.1415;
}

jn_status jn_disparity_to_u8(int32_t device, const float* dD, uint8_t* dOut, int64_t n) {
  if (!dD || !dOut || n < 0) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  if (n) launch_to_u8(nullptr, dD, dOut, n);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

jn_status jn_build_valid_disp_lut(int32_t device, const jn_scan_params* sp, int32_t W, int32_t H, uint8_t* dLut) {
  if (!sp || !dLut || W < 1 || H < 1) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  launch_valid_lut(nullptr, *sp, W, H, dLut);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

static jn_status scan_common(int32_t device, const jn_scan_params* sp, int32_t n, const float* dD, uint8_t* dDisp,
                             const uint8_t* dLut, int32_t W, int32_t H, double* dBins, double* dMeta) {
  if (!sp || !dDisp || !dBins || !dMeta || n < 1 || sp->bins < 1 || sp->bins > 1024) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  void* extrema = nullptr;                                    // [n][4] uint64
  HIP_TRY(thread_scratch(device, sizeof(unsigned long long) * 4 * (size_t)n, &extrema));
  launch_scan(nullptr, *sp, n, dD, dDisp, dLut, W, H, dBins, dMeta, static_cast<unsigned long long*>(extrema));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

jn_status jn_obstacle_scan(int32_t device, const jn_scan_params* sp, int32_t n, const uint8_t* dDisp, const uint8_t* dLut,
                           int32_t W, int32_t H, double* dBins, double* dMeta) {
  if (!dLut) return JN_ERR_INVALID;
  return scan_common(device, sp, n, nullptr, const_cast<uint8_t*>(dDisp), dLut, W, H, dBins, dMeta);
}

jn_status jn_obstacle_scan_cloud(int32_t device, const jn_scan_params* sp, int32_t n, const uint8_t* dDisp, int32_t W, int32_t H,
                                 double* dBins, double* dMeta) {
  return scan_common(device, sp, n, nullptr, const_cast<uint8_t*>(dDisp), nullptr, W, H, dBins, dMeta);
}

jn_status jn_disparity_scan(int32_t device, const jn_scan_params* sp, int32_t n, const float* dD, const uint8_t* dLut,
                            int32_t W, int32_t H, uint8_t* dDispU8, double* dBins, double* dMeta) {
  if (!dD || !dLut) return JN_ERR_INVALID;
  return scan_common(device, sp, n, dD, dDispU8, dLut, W, H, dBins, dMeta);
}

int32_t jn_compact_ranges(const double* bins, int32_t nbins, float* ranges) {
  int32_t k = 0;
  for (int i = nbins - 1; i >= 0; i--)                      // point_cloud.cpp:278-282
    if (bins[i] < JN_SCAN_EMPTY - 1) ranges[k++] = (float)bins[i];
  return k;
}

jn_status jn_point_cloud(int32_t device, const jn_scan_params* sp, const uint8_t* dDisp, int32_t W, int32_t H, float* dXyz,
                         int64_t* count) {
  if (!sp || !dDisp || !dXyz || !count || W < 1 || H < 1) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, sizeof(long long) * ((size_t)W + 1), &scratch));
  long long* cols = static_cast<long long*>(scratch);
  launch_point_cloud(nullptr, *sp, dDisp, W, H, dXyz, cols);
  long long total = 0;
  HIP_TRY(hipMemcpy(&total, cols + W, sizeof(long long), hipMemcpyDeviceToHost));
  HIP_TRY(hipGetLastError());
  *count = total;
  return JN_OK;
}

// ---- rectification front end -----------------------------------------------------------------------
jn_status jn_init_undistort_rectify_map(int32_t device, const double K[9], const double D[5], const double R[9], const double P[12],
                                        int32_t W, int32_t H, float* dMapX, float* dMapY) {
  if (!K || !D || !R || !P || !dMapX || !dMapY || W < 1 || H < 1) return JN_ERR_INVALID;
  // iR = inverse(P[:, :3] * R), by cofactors
  double M[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) M[3 * i + j] = P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j] + P[4 * i + 2] * R[6 + j];
  const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
  if (det == 0.0) return JN_ERR_INVALID;
  const double id = 1.0 / det;
  const double iR[9] = {c00 * id, (M[2] * M[7] - M[1] * M[8]) * id, (M[1] * M[5] - M[2] * M[4]) * id,
                        c01 * id, (M[0] * M[8] - M[2] * M[6]) * id, (M[2] * M[3] - M[0] * M[5]) * id,
                        c02 * id, (M[1] * M[6] - M[0] * M[7]) * id, (M[0] * M[4] - M[1] * M[3]) * id};
  HIP_TRY(hipSetDevice(device));
  launch_undistort_map(nullptr, iR, K, D, W, H, dMapX, dMapY);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

jn_status jn_remap_bilinear(int32_t device, int32_t n, const uint8_t* dSrc, int32_t sw, int32_t sh, int32_t spitch, int64_t sstride,
                            const float* dMapX, const float* dMapY, uint8_t* dDst, int32_t W, int32_t H, int32_t dpitch, int64_t dstride) {
  if (!dSrc || !dMapX || !dMapY || !dDst || n < 1 || sw < 1 || sh < 1 || W < 1 || H < 1 || spitch < sw || dpitch < W) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  launch_remap(nullptr, n, dSrc, sw, sh, spitch, sstride, dMapX, dMapY, dDst, W, H, dpitch, dstride);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // extern "C"

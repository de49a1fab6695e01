// elas_seams.cpp — single stages of the ELAS path behind C entry points of their own (include/jn_stereo.h): the host stage and its
// triangulation, and the device's arrangement, triangulation and support filters on caller-supplied data.  What the tests compare stage
// by stage; no handle, no slot.  Product code.
#include "../../include/jn_stereo.h"
#include "hooks.h"
#include "hip_try.h"
#include "kernels.h"
#include "host_stage.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

using namespace jnav;

extern "C" {

// ---- host-stage hooks -----------------------------------------------------------------------------
int32_t jn_host_triangulate(const int32_t* x, const int32_t* y, int32_t n, int32_t* tri) {
  if (!x || !y || !tri || n < 0) return -1;
  Delaunay dt;
  return dt.run(x, y, n, tri);
}

int32_t jn_host_triangulate_parts(const int32_t* x, const int32_t* y, int32_t n, int32_t* tri, int32_t parts) {
  if (!x || !y || !tri || n < 0) return -1;
  Delaunay dt;
  const int got = dt.prepare(x, y, n, parts);
  if (got == 0) return -1;
  std::vector<std::thread> th;                               // the parts really run concurrently
  for (int i = 1; i < got; i++) th.emplace_back([&dt, i] { dt.subtree(i); });
  dt.subtree(0);
  for (auto& t : th) t.join();
  return dt.finish(tri);
}

int32_t jn_host_arrangement(const int32_t* x, const int32_t* y, int32_t n, uint16_t* out) {
  if (!x || !y || !out || n < 0) return -1;
  Delaunay dt;
  return dt.arrangement(x, y, n, out) ? 1 : 0;
}

// bounds of a list of (uc, vc, d) triples for k_arrange's rank form (the product passes what the handle's lattice and disparity range give)
static bool arrange_by_sorts() { const char* e = JN_HOOK_ENV("JN_ARRANGE_SORTS"); return e && atoi(e) != 0; }   // hooks build: the sort forms where the rank form would run
static ArrBounds bounds_of(const int16_t* t, int n, int step) {
  if (n <= 0 || arrange_by_sorts()) return ArrBounds{0, 0, 0, 0};
  int ucm = 0, vcm = 0, xlo = 1 << 30, xhi = -(1 << 30);
  for (int i = 0; i < n; i++) {
    const int uc = t[3 * i], vc = t[3 * i + 1], x = uc * step - t[3 * i + 2];
    if (uc < 0 || vc < 0) return ArrBounds{0, 0, 0, 0};
    ucm = std::max(ucm, uc); vcm = std::max(vcm, vc); xlo = std::min(xlo, x); xhi = std::max(xhi, x);
  }
  return ArrBounds{vcm + 1, ucm + 1, xlo, xhi - xlo + 1};
}
jn_status jn_device_arrangement(int32_t device, const int16_t* triples, int32_t n, int32_t step, uint16_t* left, uint16_t* right,
                                int32_t ok[2]) {
  if (!triples || !left || !right || !ok || n < 0 || step < 1) return JN_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return JN_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(configure_device_kernels());
  const int cap = std::max(n, 1), arr_cap = std::min(cap, 8192), g_cap = std::min(cap, 16384);
  int16_t* d_list = nullptr; int32_t* d_cnt = nullptr; uint16_t* d_arr = nullptr; int32_t* d_ok = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_list), (size_t)cap * 3 * sizeof(int16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_cnt), sizeof(int32_t));
  void* d_scratch = nullptr;
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_arr), (size_t)2 * g_cap * sizeof(uint16_t));
  if (e == hipSuccess && g_cap > arr_cap) e = hipMalloc(&d_scratch, arrange_scratch_bytes(1, g_cap));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_ok), 2 * sizeof(int32_t));
  if (e == hipSuccess && n) e = hipMemcpy(d_list, triples, (size_t)n * 3 * sizeof(int16_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cnt, &n, sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) { launch_arrange(nullptr, 1, d_list, d_cnt, cap, step, arr_cap, g_cap, d_arr, d_ok, d_scratch, d_scratch ? g_cap : 0, bounds_of(triples, n, step)); e = hipStreamSynchronize(nullptr); }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(ok, d_ok, 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && ok[0]) e = hipMemcpy(left, d_arr, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess && ok[1]) e = hipMemcpy(right, d_arr + g_cap, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost);
  hipFree(d_list); hipFree(d_cnt); hipFree(d_arr); hipFree(d_ok); hipFree(d_scratch);
  HIP_TRY(e);
  return JN_OK;
}

jn_status jn_device_triangulate(int32_t device, const int16_t* triples, int32_t n, int32_t step, int32_t* tri_left, int32_t* tri_right, int32_t ntri[2],
                                int32_t* need_host) {
  if (!triples || !tri_left || !tri_right || !ntri || !need_host || n < 0 || step < 1) return JN_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return JN_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(configure_device_kernels());
  const int cap = std::max(n, 1), arr_cap = std::min(cap, 8192), g_cap = std::min(cap, 16384);
  const int whole = delaunay_gpu_capacity(152 * 1024);
  const size_t pay = (size_t)cap * 12 + 2 * (2 * (size_t)cap + 8) * 12 + 256;
  int16_t* d_list = nullptr; int32_t* d_cnt = nullptr; uint16_t* d_arr = nullptr; int32_t* d_ok = nullptr; uint8_t* d_pay = nullptr; FrameInfo* d_info = nullptr; int32_t* d_need = nullptr;
  void* d_ascr = nullptr; uint8_t* d_dscr = nullptr;            // more vertices than the LDS forms take: the arrangement's and the triangulation's global scratch
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_list), (size_t)cap * 3 * sizeof(int16_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_cnt), sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_arr), (size_t)2 * g_cap * sizeof(uint16_t));
  if (e == hipSuccess && g_cap > arr_cap) e = hipMalloc(&d_ascr, arrange_scratch_bytes(1, g_cap));
  if (e == hipSuccess && n > whole) e = hipMalloc(reinterpret_cast<void**>(&d_dscr), delaunay_gpu_scratch_bytes(1, g_cap));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_ok), 2 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_pay), pay);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_info), sizeof(FrameInfo));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_need), sizeof(int32_t));
  if (e == hipSuccess && n) e = hipMemcpy(d_list, triples, (size_t)n * 3 * sizeof(int16_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cnt, &n, sizeof(int32_t), hipMemcpyHostToDevice);
  FrameInfo fi;
  memset(&fi, 0, sizeof(fi));
  if (e == hipSuccess) {
    launch_arrange(nullptr, 1, d_list, d_cnt, cap, step, arr_cap, g_cap, d_arr, d_ok, d_ascr, d_ascr ? g_cap : 0, bounds_of(triples, n, step));
    long long* d_clk = nullptr;
    const bool want_clk = JN_HOOK_ENV("JN_DT_CLOCKS") != nullptr;
    if (want_clk && hipMalloc(reinterpret_cast<void**>(&d_clk), 64 * sizeof(long long)) == hipSuccess) hipMemset(d_clk, 0, 64 * sizeof(long long));
    bool wide = false;                                       // coordinates beyond (-2048, 2048): the integer predicates
    for (int i = 0; i < n; i++) wide |= triples[3 * i] * step >= 2048 || triples[3 * i + 1] * step >= 2048;
    launch_delaunay(nullptr, 1, d_list, d_cnt, cap, step, d_arr, d_ok, g_cap, d_dscr ? n : whole, d_pay, (long long)pay, d_info, d_need, d_clk, d_dscr, d_dscr ? g_cap : 0, 0, wide);
    e = hipStreamSynchronize(nullptr);
    if (d_clk) {                                             // JN_DT_CLOCKS: microseconds per tree level (leaves first) of both sides, to stderr
      long long clk[64];
      if (hipMemcpy(clk, d_clk, sizeof(clk), hipMemcpyDeviceToHost) == hipSuccess)
        for (int sd = 0; sd < 2; sd++) {
          fprintf(stderr, "k_delaunay n=%d side %d, us per level from the leaves up:", n, sd);
          long long prev = clk[sd * 32 + 31];
          for (int k = 30; k >= 0; k--) if (clk[sd * 32 + k]) { fprintf(stderr, " %.1f", (clk[sd * 32 + k] - prev) / 100.0); prev = clk[sd * 32 + k]; }
          fprintf(stderr, "  total %.1f\n", (prev - clk[sd * 32 + 31]) / 100.0);
        }
      hipFree(d_clk);
    }
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(&fi, d_info, sizeof(fi), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(need_host, d_need, sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    ntri[0] = fi.ntri[0]; ntri[1] = fi.ntri[1];
    if (fi.ntri[0] > 0) e = hipMemcpy(tri_left, d_pay + fi.corner_offset[0], (size_t)fi.ntri[0] * 12, hipMemcpyDeviceToHost);
    if (e == hipSuccess && fi.ntri[1] > 0) e = hipMemcpy(tri_right, d_pay + fi.corner_offset[1], (size_t)fi.ntri[1] * 12, hipMemcpyDeviceToHost);
  }
  hipFree(d_list); hipFree(d_cnt); hipFree(d_arr); hipFree(d_ok); hipFree(d_pay); hipFree(d_info); hipFree(d_need); hipFree(d_ascr); hipFree(d_dscr);
  HIP_TRY(e);
  return JN_OK;
}

jn_status jn_device_support_filters(int32_t device, const jn_elas_params* p, int32_t W, int32_t H, int32_t n, int16_t* d_can,
                                    int32_t form) {
  if (!p || !d_can || n < 1 || W < 1 || H < 1 || p->candidate_stepsize < 1 || form < 0 || form > 2) return JN_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return JN_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(configure_device_kernels());
  DevParams dp;
  memset(&dp, 0, sizeof(dp));
  dp.W = W; dp.H = H; dp.step = p->candidate_stepsize;
  dp.cw = (W + dp.step - 1) / dp.step; dp.ch = (H + dp.step - 1) / dp.step;
  const size_t cells = (size_t)n * dp.cw * dp.ch;
  if (form == 2 && !support_filters_fast(dp, p->incon_window_size, p->incon_min_support)) return JN_ERR_UNSUPPORTED;
  int16_t* d = nullptr; uint8_t* scratch = nullptr;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), cells * sizeof(int16_t)));
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&scratch), cells);
  if (e != hipSuccess) { hipFree(d); HIP_TRY(e); }
  e = hipMemcpy(d, d_can, cells * sizeof(int16_t), hipMemcpyHostToDevice);
  bool ran = false;
  if (e == hipSuccess) {
    ran = launch_support_filters(nullptr, dp, n, p->incon_window_size, p->incon_threshold, p->incon_min_support, d,
                                 form == 1 ? nullptr : scratch);       // no scratch: only the wavefront kernel can run
    if (ran) e = hipMemcpy(d_can, d, cells * sizeof(int16_t), hipMemcpyDeviceToHost);
  }
  hipFree(d); hipFree(scratch);
  HIP_TRY(e);
  HIP_TRY(hipGetLastError());
  return ran ? JN_OK : JN_ERR_UNSUPPORTED;
}

static_assert(sizeof(jn_host_frame_info) == sizeof(FrameInfo), "jn_host_frame_info mirrors FrameInfo");

int64_t jn_host_stage(const jn_elas_params* p, int32_t W, int32_t H, int16_t* d_can, uint8_t* payload, int64_t payload_cap,
                      jn_host_frame_info* info) {
  if (!p || !d_can || !payload || !info || p->candidate_stepsize < 1 || p->grid_size < 1) return -1;
  HostParams hp;
  hp.W = W; hp.H = H; hp.disp_max = p->disp_max; hp.step = p->candidate_stepsize;
  hp.incon_window_size = p->incon_window_size; hp.incon_threshold = p->incon_threshold;
  hp.incon_min_support = p->incon_min_support; hp.grid_size = p->grid_size;
  hp.gw = (int)std::ceil((float)W / (float)p->grid_size); hp.gh = (int)std::ceil((float)H / (float)p->grid_size);
  hp.cw = (W + hp.step - 1) / hp.step; hp.ch = (H + hp.step - 1) / hp.step;
  hp.add_corners = p->add_corners ? 1 : 0;
  if ((int64_t)HostWorker::payload_capacity(hp) > payload_cap) return -1;
  HostWorker w(hp);
  FrameInfo fi;
  FrameScratch fs;
  w.filter_and_list(d_can, &fi, &fs);
  HostWorker::place(&fi, 0);
  w.triangulate_side(0, fs, payload, &fi);
  w.triangulate_side(1, fs, payload, &fi);
  memcpy(info, &fi, sizeof(fi));
  return fi.ok ? fi.corner_offset[1] + (int64_t)fi.ntri[1] * 3 * (int64_t)sizeof(int32_t) : 0;
}

}  // extern "C"

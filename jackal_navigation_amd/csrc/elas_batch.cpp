// elas_batch.cpp — what a slot's worker does with one ELAS batch (the handle and its slots: elas_handle.h; the calls that feed them:
// elas_api.cpp).  Product code.
//
// Pipeline per batch (one "slot" = one HIP stream + its buffers + one worker thread):
//   GPU stage A : Sobel planes -> support matching -> support filters -> support list -> alternating-cut arrangement   (kernels.hip)
//                 the list (uc, vc, d) is written by the GPU straight into pinned host memory
//   host stage  : Delaunay's hull recursion x2 per frame                       (delaunay.cpp, thread pool)
//                 (+ the support filters when no kernel takes the lattice or JN_HOST_FILTERS=1: host_stage.cpp)
//   H2D         : one copy per batch: support points + triangle corner indices
//   GPU stage B : grid prior, plane fits, raster bins, ownership -> dense L/R -> L/R check -> speckle -> gaps -> adaptive mean
//                 [-> u8 map + obstacle scan when submitted through jn_elas_submit_scan]
// Several slots in flight overlap one batch's host stage with another batch's GPU stages.
// Batch handles of processes with few cores of their own have NO host stage: the hull recursion runs on the GPU too (delaunay_gpu.hip),
// FrameInfo and the payload are written on the device and stage B is queued right behind it (finish_gpu_route).
#include "elas_handle.h"
#include "hooks.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include <pthread.h>
#include <sys/prctl.h>

using namespace jnav;

namespace {

// Waiting for the GPU without burning the host's cores.  hipEventSynchronize spins on this runtime even for events created
// with hipEventBlockingSync: the four slot workers then cost 2.5 cores of pure waiting (measured: 4.2 ms of CPU per 32-pair
// batch), and on the GPU boxes the container's CPU quota (16 CPUs) is what the Delaunay pool needs.  So: poll the event —
// tightly for the first 60 us, then between short sleeps (a batch's stage lasts milliseconds; the other slots keep the GPU
// busy meanwhile).  A latency-mode handle (max_batch 1) polls tightly for 1 ms: its stages are short and a sleep's wake-up
// would show in every call.  JN_WAIT_SPIN_US overrides (-1: plain hipEventSynchronize).
// With a deadline (timeout_ms > 0): hipErrorNotReady when it passed without the event completing.
hipError_t wait_event(hipEvent_t ev, int spin_us, int timeout_ms = 0) {
  if (spin_us < 0 && timeout_ms <= 0) return hipEventSynchronize(ev);
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    const auto waited = std::chrono::steady_clock::now() - t0;
    if (timeout_ms > 0 && waited > std::chrono::milliseconds(timeout_ms)) return hipErrorNotReady;
    if (waited < std::chrono::microseconds(spin_us)) { __builtin_ia32_pause(); continue; }
    std::this_thread::sleep_for(std::chrono::microseconds(waited < std::chrono::microseconds(500) ? 20 : 50));
  }
}

// Parts a triangulation is cut into on the host: idle pool threads (a lone pair, a few large frames) are put to work inside it.
int delaunay_parts(const jn_elas* h, int n) {
  const int threads = h->pool->size();
  return h->split_delaunay ? (threads >= 8 * n ? 4 : (threads >= 4 * n ? 2 : 1)) : 1;
}

// A scan batch that carries a merge owns one place in the handle's merge order.  If the batch ends early (a HIP error on the
// way), the place must still be given up, or every later batch of this handle would wait for it for ever — and the OTHER ranks
// of the communicator are inside, or about to enter, the same all-reduce: this rank still takes part in it, contributing the
// identity of MIN (comm_merge_identity), so the peers get the remaining rigs' scan while this rank reports its error.
struct MergeTurn {
  jn_elas* h; uint64_t seq; bool armed; int n, bins;
  MergeTurn(jn_elas* h_, const Job& j) : h(h_), seq(j.seq), armed(j.merge), n(j.n), bins(j.sp.bins) {}
  void done() { armed = false; }
  ~MergeTurn() {
    if (!armed) return;
    {
      std::unique_lock<std::mutex> l(h->merge_m);
      h->merge_cv.wait(l, [&] { return h->merge_seq == seq; });
      if (h->comm) comm_merge_identity(h->comm, n, bins);
      if (h->merge_log.size() >= 4096) h->merge_log.erase(h->merge_log.begin(), h->merge_log.begin() + 2048);
      h->merge_log.push_back(seq);
      h->merge_seq++;
    }
    h->merge_cv.notify_all();
  }
};

// Latency mode (a handle of max_batch 1): a lone pair's stage B is two dozen launches of a few microseconds each, and queued after the
// host stage they reach the GPU slower than it finishes them (~30 us of idle gaps at 640x480).  They are queued while the GPU runs
// stage A instead, behind a wait on a word of signal memory that the host sets when its stage is done (hipStreamWaitValue32).  What
// the host stage decides is then not known at launch time: the three launches sized by support / triangle counts take their capacity
// (the kernels return on indices beyond the frame's counts), the payload and FrameInfo are read where the host will have written them,
// and the two clears that depend on nothing run ahead of the gate.  Whatever happens afterwards, the gate is opened (GateGuard): a
// stream left waiting would hang the handle.
struct GateGuard {
  volatile uint32_t* word = nullptr; uint32_t value = 0;
  FrameInfo* info = nullptr; int n = 0; hipStream_t st = nullptr;
  bool shut() const { return word != nullptr; }
  void open() { if (word) { std::atomic_thread_fence(std::memory_order_seq_cst); *word = value; word = nullptr; } }
  // An early return with the gate still shut: stage B is on the stream and WILL run once the gate opens, on whatever FrameInfo holds —
  // the previous batch's, if the host stage never ran.  Every frame is therefore marked as failed first (the matching and the
  // post-processing return on !ok; the scan tail still scans whatever D1 holds into the caller's buffers), and the stream is drained
  // before the error goes back: the caller may free its buffers as soon as it has it.
  ~GateGuard() {
    if (!word) return;
    for (int i = 0; i < n; i++) info[i].ok = 0;
    open();
    hipStreamSynchronize(st);
  }
};

// What stage A decided while it was queued.
struct StageA {
  bool filtered = false;                                 // the device filters ran: the GPU lists the support points itself
  bool arranged = false;                                 // k_arrange was launched for the triangulations to start from
  bool gpu_dt = false;                                   // k_delaunay was launched: no host stage
  bool grid_early = false;                               // the candidate grid is queued already
};

// Stage B as a function of what the host stage yields.
struct StageBInput {
  int max_sup, max_tri;                                  // the largest support / triangle counts (launch sizes), or their capacities where the counts are not known yet
  bool any_ok;                                           // some frame has a triangulation
  const uint8_t* payload; size_t payload_bytes;          // where the payload is read from: s.payload (and the bytes to copy there first) or pinned memory
  bool cleared;                                          // the two clears were queued ahead
  bool device_info;                                      // FrameInfo was written on the device: nothing to copy
};

// What the route of one pass leaves for run_batch.
struct RouteResult {
  std::chrono::steady_clock::time_point t_begin;
  float host_ms = 0.f;                                   // the host stage on the worker's clock
  bool any_ok = false;
  bool handed_back = false;                              // GPU route: k_delaunay left a side to the host, the batch goes through the host route
};

// What one pass of a batch over a route works on.  Everything here is fixed before anything is queued; what only becomes known while
// queueing is returned by the stage that decides it (StageA; the host stage's part of StageBInput).
struct Batch {
  jn_elas* h; Slot& s; const Job& j; const DevParams& dp;
  int n;
  // Stage A (descriptors -> support matches -> filters -> list -> arrangement) ends in the host stage, which the whole batch
  // waits for; its small kernels (one workgroup per frame or side) would otherwise queue behind the dense kernels of the
  // other slots.  It runs on a stream of the highest priority; stage B stays on the slot's ordinary stream.  The two never
  // overlap within a slot (the worker waits for stage A, and for the batch's end before the next stage A), so no events tie
  // them together.  Host-pointer jobs stage their images on the ordinary stream and keep everything there.
  hipStream_t st, sa;
  DescSrc dsrc;
  // Stage boundaries for jn_elas_last_times.  A timing event between two kernels costs ~6 us of idle GPU: nothing when
  // other slots fill the gap, 7 % of a lone 640x480 pair — a latency-mode handle (max_batch 1) leaves them out.
  bool stage_events;
  // the plan: the route decisions that do not depend on what the kernels find
  int list_cap;                                          // support points a frame can hold: the lattice
  // Where the list and the arrangement live: in device memory when this batch is going to triangulate on the GPU (everything that decides
  // it is known here except whether the filter kernel lists the points itself: if it does not, the list goes to pinned memory and the host
  // route is taken), in pinned host memory for the host stage.
  bool want_gpu_dt;
  int16_t* list_buf; int32_t* cnt_buf; uint16_t* arr_buf; int32_t* arr_ok_buf;
  bool fused;                                            // gap interpolation and adaptive mean as one pass
  bool grid_early_ok;                                    // the candidate grid may be queued behind stage A (see queue_stage_a)

  hipError_t mark(int e) const { return stage_events ? hipEventRecord(s.ev[e], st) : hipSuccess; }
  hipError_t mark_a(int e) const { return stage_events ? hipEventRecord(s.ev[e], sa) : hipSuccess; }
  // one pass of the post-processing over the left map and, unless the parameters ask for the left one only, the right map
  template <typename Pass>
  void each_map(Pass&& pass) const { pass(j.dD1); if (!h->p.postprocess_only_left) pass(j.dD2); }

  jn_status queue_stage_a(StageA* out) const;
  jn_status queue_post_processing() const;
  jn_status queue_stage_b(const StageA& a, const StageBInput& in) const;
  jn_status queue_gated_stage_b(const StageA& a, GateGuard& gate, bool* cleared) const;
  StageBInput host_stage(const StageA& a, float* ms) const;
  jn_status finish_gpu_route(const StageA& a, RouteResult* out) const;
  jn_status finish_host_route(const StageA& a, RouteResult* out) const;
};

// force_host: the triangulations on the host (the route of latency-mode handles, of parameter sets with corner points, and the second pass
// of a batch whose frames the GPU's triangulation handed back)
Batch plan_batch(jn_elas* h, Slot& s, const Job& j, bool force_host) {
  const DevParams& dp = h->dp;
  hipStream_t st = s.stream, sa = (s.stream_a && !j.staged) ? s.stream_a : st;
  const bool want_gpu_dt = h->gpu_delaunay && !force_host && sa == st && s.d_list &&
                           s.arr_hint <= (s.dt_scratch ? h->dt_gcap : delaunay_gpu_capacity(152 * 1024)) && h->gpu_arrange && s.arr_hint <= h->arr_stride;
  static const bool grid_early_env = !(getenv("JN_GRID_EARLY") && atoi(getenv("JN_GRID_EARLY")) == 0);
  return Batch{h, s, j, dp, j.n, st, sa,
               h->plane_flow ? DescSrc{s.planes, plane_pitch(dp.W), true} : DescSrc{s.desc, 0, false},
               h->stage_events, dp.cw * dp.ch, want_gpu_dt,
               want_gpu_dt ? s.d_list : s.h_list, want_gpu_dt ? s.d_cnt : s.h_cnt, want_gpu_dt ? s.d_arr : s.h_arr, want_gpu_dt ? s.d_arr_ok : s.h_arr_ok,
               gap_mean_fusable(dp, j.n) && ((dp.W * dp.H) & 3) == 0,
               grid_early_env && !dp.add_corners && sa == st};
}

// Pacing, Sobel planes or descriptors, support matches, device filters, list, arrangement, triangulation or the candidates' copy to the
// host, up to EV_D2H; behind it the candidate grid where it needs nothing of the host stage.
jn_status Batch::queue_stage_a(StageA* out) const {
  {
    std::unique_lock<std::mutex> pl(h->pace_m, std::defer_lock);
    if (h->pace) {
      pl.lock();
      if (h->pace_prev && h->pace_prev != s.ev_head) HIP_TRY(hipStreamWaitEvent(sa, h->pace_prev, 0));
    }
    HIP_TRY(mark_a(EV_BEGIN));
    if (h->plane_flow) launch_sobel_planes(sa, dp, j.dI1, j.dI2, j.pitch, j.stride, n, s.planes);
    else launch_descriptor(sa, dp, j.dI1, j.dI2, j.pitch, j.stride, n, s.desc);
    HIP_TRY(mark_a(EV_DESC));
    launch_support(sa, dp, n, dsrc, s.d_can);
    if (h->pace) { HIP_TRY(hipEventRecord(s.ev_head, sa)); h->pace_prev = s.ev_head; }
  }
  bool listed = false;                                   // k_filter_resolve wrote the support list too
  const bool filtered = (n >= h->filter_min_batch || (h->filter_min_batch < (1 << 30) && h->filters_fast)) &&
      launch_support_filters(sa, dp, n, h->p.incon_window_size, h->p.incon_threshold, h->p.incon_min_support, s.d_can, s.tmp, list_buf, cnt_buf, list_cap, &listed);
  HIP_TRY(mark_a(EV_SUPPORT));
  bool arranged = false, gpu_dt = false;
  if (filtered) {                                        // the GPU lists the support points itself (into pinned host memory for the host stage)
    if (!listed) { launch_support_list(sa, dp, n, s.d_can, list_buf, cnt_buf, list_cap); listed = true; }
    // the arrangement the triangulations start from, unless the pool has idle threads and will cut them into parts itself
    // Sized by what this slot's previous batch held (+25 %): a 720p frame has 3.2 k support points and needs 52 KB of LDS, not
    // the 104 KB of the 8192-vertex maximum — a workgroup that asks for less finds room among the other slots' kernels sooner.
    // Frames beyond the maximum (1920x1080: 11 k points) skip the launch: it could only hand every side back.
    // The triangulation itself on the GPU (delaunay_gpu.hip) wherever it applies: batch handles, no corner points, lattices the LDS holds.
    // Then there is NO host stage: k_delaunay writes FrameInfo and the payload on the device, stage B is queued right behind it with
    // capacity-sized launches, and the worker only waits for the batch's end.
    gpu_dt = want_gpu_dt && listed;
    arranged = h->gpu_arrange && (gpu_dt || delaunay_parts(h, n) == 1) && s.arr_hint <= h->arr_stride;
    if (arranged) {
      const int want = s.arr_hint ? s.arr_hint + s.arr_hint / 4 + 64 : h->arr_cap;
      // more points than the LDS can order (1920x1080: 11 k): every side works in its slice of the global scratch, the launch asks for the minimum of LDS
      const int cap = s.arr_hint > h->arr_cap ? 1024 : std::min(h->arr_cap, std::max(1024, (want + 1023) / 1024 * 1024));
      // (the global-scratch form only when the slot's recent batches held a side beyond the LDS form: at 1280x720 it would be an empty launch per batch)
      const bool big = s.arr_scratch && (s.arr_hint == 0 || s.arr_hint > h->arr_cap);   // (0: the slot's first batch — nothing known yet)
      launch_arrange(sa, n, list_buf, cnt_buf, list_cap, dp.step, cap, h->arr_stride, arr_buf, arr_ok_buf, big ? s.arr_scratch : nullptr, big ? h->arr_stride : 0,
                     h->arrange_sorts ? ArrBounds{0, 0, 0, 0} : ArrBounds{dp.ch, dp.cw, -dp.disp_max, (dp.cw - 1) * dp.step + dp.disp_max + 1});
      if (gpu_dt)                                        // LDS for what the slot's last batches held + 6 % (a tight request: 32 bytes a vertex leave a k_dense_row workgroup room on the same CU); a side beyond it goes to the host
        HIP_TRY(launch_delaunay(sa, n, list_buf, cnt_buf, list_cap, dp.step, arr_buf, arr_ok_buf, h->arr_stride, s.arr_hint ? std::max(1024, s.arr_hint + s.arr_hint / 16 + 32) : (1 << 30), s.payload,
                                (long long)h->payload_cap, s.info, s.need_host, nullptr, s.dt_scratch, h->dt_gcap, s.arr_hint, dp.W >= 2048 || dp.H >= 2048));
    }
  } else {
    const size_t can_bytes = (size_t)dp.cw * dp.ch * sizeof(int16_t);
    HIP_TRY(hipMemcpyAsync(s.h_can, s.d_can, can_bytes * n, hipMemcpyDeviceToHost, sa));
  }
  HIP_TRY(hipEventRecord(s.ev[EV_D2H], sa));
  // The candidate grid (elas.cpp:582-680) needs the support points, not the triangulation: without corner points they are the list the
  // GPU has just written, so the grid is queued HERE, behind stage A, and is built while the host triangulates (JN_GRID_EARLY=0: in stage B).
  const bool grid_early = grid_early_ok && filtered;
  if (grid_early) launch_grid_from_list(st, dp, n, list_buf, cnt_buf, list_cap, s.mark, s.gridbits);
  *out = StageA{filtered, arranged, gpu_dt, grid_early};
  return JN_OK;
}

// Post-processing, raw matcher output -> D1 / D2.  When gap interpolation and adaptive mean can run as one pass (gap_mean_fusable), the
// left image travels raw -> tmp (L/R check) -> tmp (speckle, run lists in the still idle output image) -> D1 (fused pass), so that
// every stage reads and writes the image once; otherwise the stages run in place on D1 with tmp as scratch.
jn_status Batch::queue_post_processing() const {
  const bool only_left = h->p.postprocess_only_left != 0, mean = h->p.filter_adaptive_mean != 0;
  if (h->sub) {
    // subsampling: the matcher ran on every pixel (findMatch is per pixel, so the reference's half-size map is the full one at even
    // (u, v)); the L/R check picks those out, everything behind it works on (W/2) x (H/2) maps with dph
    const DevParams& dph = h->dph;
    launch_lr_sub(st, dp, n, s.info, s.raw, j.dD1, j.dD2);
    HIP_TRY(mark(EV_LR));
    each_map([&](float* D) { launch_speckle(st, dph, n, s.info, D, s.label, s.size, s.tmp); });
    HIP_TRY(mark(EV_SPECKLE));
    each_map([&](float* D) { launch_gap(st, dph, n, s.info, D, s.tmp); });
    HIP_TRY(mark(EV_GAP));
    if (mean) each_map([&](float* D) { launch_adaptive_mean_sub(st, dph, n, s.info, D, s.tmp); });
    if (h->p.filter_median) each_map([&](float* D) { launch_median(st, dph, n, s.info, D, s.tmp); });
    HIP_TRY(mark(EV_AM));
    return JN_OK;
  }
  if (fused) {
    launch_lr_speckle(st, dp, n, s.info, s.raw, s.tmp, j.dD2, s.label, s.size, j.dD1);   // (the L/R check and the speckle pass' row labelling are one kernel here)
    HIP_TRY(mark(EV_LR));
    HIP_TRY(mark(EV_SPECKLE));
    launch_gap_mean_fused(st, dp, n, s.info, s.tmp, j.dD1, mean);
    if (!only_left) {                                    // right image: in place, fused pass into tmp, copied back
      launch_speckle(st, dp, n, s.info, j.dD2, s.label, s.size, s.tmp);
      launch_gap_mean_fused(st, dp, n, s.info, j.dD2, s.tmp, mean);
      launch_copy_ok(st, dp, n, s.info, s.tmp, j.dD2);
    }
    HIP_TRY(mark(EV_GAP));
  } else {
    launch_lr_speckle(st, dp, n, s.info, s.raw, j.dD1, j.dD2, s.label, s.size, s.tmp);   // L/R check of both maps + the left map's speckle pass (its row labelling in the L/R kernel)
    HIP_TRY(mark(EV_LR));
    if (!only_left) launch_speckle(st, dp, n, s.info, j.dD2, s.label, s.size, s.tmp);
    HIP_TRY(mark(EV_SPECKLE));
    each_map([&](float* D) { launch_gap(st, dp, n, s.info, D, s.tmp); });
    HIP_TRY(mark(EV_GAP));
    if (mean) each_map([&](float* D) { launch_adaptive_mean(st, dp, n, s.info, D, s.tmp); });
  }
  if (h->p.filter_median) each_map([&](float* D) { launch_median(st, dp, n, s.info, D, s.tmp); });   // elas.cpp:133-139
  HIP_TRY(mark(EV_AM));
  return JN_OK;
}

// H2D copies, grid / bins / dense matching, post-processing, the scan and the attached tails, EV_END.
jn_status Batch::queue_stage_b(const StageA& a, const StageBInput& in) const {
  HIP_TRY(mark(EV_H2D0));
  if (!in.device_info) HIP_TRY(hipMemcpyAsync(s.info, s.h_info, sizeof(FrameInfo) * n, hipMemcpyHostToDevice, st));
  if (in.payload_bytes && in.payload == s.payload) HIP_TRY(hipMemcpyAsync(s.payload, s.h_payload, in.payload_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(mark(EV_H2D));
  if (in.any_ok) {
    if (!a.grid_early) launch_grid(st, dp, n, s.info, in.payload, 0, in.max_sup, s.mark, s.gridbits, !in.cleared);      // offsets in FrameInfo are batch-absolute
    launch_bin(st, dp, n, s.info, s.recs, h->tri_cap, in.max_tri, s.bin_count, s.bin_list, !in.cleared, in.payload, 0);   // (forms the triangles' records on the way: k_tri_setup's work)
    HIP_TRY(mark(EV_RASTER));
    launch_dense(st, dp, n, s.info, s.recs, h->tri_cap, s.bin_count, s.bin_list, s.gridbits, dsrc, s.raw, false, (stage_events && h->plane_flow) ? s.ev_owner : nullptr);
    HIP_TRY(mark(EV_DENSE));
    const jn_status ps = queue_post_processing();
    if (ps != JN_OK) return ps;
  } else {
    for (int e = EV_RASTER; e <= EV_AM; e++) HIP_TRY(mark(e));
  }
  if (j.scan) {
    // the node's tail: depth map + obstacle scan of whatever D1 now holds
    launch_scan(st, j.sp, n, j.dD1, j.dDispU8, j.dLut, dp.W, dp.H, j.dBins, j.dMeta, s.scan_scratch, j.merge ? s.d_flat : nullptr);
    // the attached tails: the costmap of the map and the bins the scan has just written, the sub-pixel tail of the float map
    const int native = JN_DISP_F32;
    HIP_TRY(j.tails.launch(st, j.sp, n, j.dDispU8, j.dLut, j.dBins, j.dD1, native, dp.W, dp.H));
  }
  HIP_TRY(hipEventRecord(s.ev[EV_END], st));
  return JN_OK;
}

// The most support points a frame of the slot's last kArrHist batches held: the next batch's arrangement space and LDS requests (a lone
// sparse frame no longer shrinks them).
void note_support_counts(Slot& s, int batch_most) {
  s.arr_hist[s.arr_pos] = batch_most; s.arr_pos = (s.arr_pos + 1) % Slot::kArrHist;
  s.arr_hint = *std::max_element(s.arr_hist, s.arr_hist + Slot::kArrHist);
}

// The GPU route behind stage A: stage B with capacity-sized launches, one wait, and what the host needs of the batch.
jn_status Batch::finish_gpu_route(const StageA& a, RouteResult* out) const {
  out->any_ok = true;
  const jn_status qs = queue_stage_b(a, StageBInput{list_cap, h->tri_cap, true, s.payload, 0, false, true});
  if (qs != JN_OK) return qs;
  // what the host needs of the batch: which frames matched out (status), how many support points they held (the next launches' LDS),
  // whether a side was handed back — copied behind everything else, read after the one wait
  HIP_TRY(hipMemcpyAsync(s.h_info, s.info, sizeof(FrameInfo) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s.h_need, s.need_host, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipEventRecord(s.ev[EV_END], st));
  HIP_TRY(wait_event(s.ev[EV_END], h->wait_spin_us));
  HIP_TRY(hipGetLastError());
  int batch_most = 0, handed_back = 0;
  for (int i = 0; i < n; i++) { batch_most = std::max(batch_most, (int)s.h_info[i].reserved); handed_back |= s.h_need[i]; }   // (k_delaunay leaves the frame's support count, clipped or not, in `reserved`)
  note_support_counts(s, batch_most);
  out->handed_back = handed_back != 0;                   // coinciding vertices or more of them than the launch's LDS held: the whole batch again, host stage and all
  if (!handed_back)
    for (int i = 0; i < n; i++) if (j.status) j.status[i] = s.h_info[i].ok ? JN_OK : JN_ERR_FEW_SUPPORT;
  return JN_OK;
}

// Latency mode: the two clears and the whole of stage B behind a shut gate, while the GPU runs stage A (see GateGuard).  *cleared: the
// clears are on the stream, whether or not the gate could be shut behind them.
jn_status Batch::queue_gated_stage_b(const StageA& a, GateGuard& gate, bool* cleared) const {
  *cleared = false;
  if (!(h->gate_stage_b && s.gate && a.filtered && h->zero_copy_payload && sa == st)) return JN_OK;
  if (!a.grid_early) launch_grid_clear(st, dp, n, s.mark);
  launch_bin_clear(st, dp, n, s.bin_count);
  *cleared = true;
  const uint32_t v = ++s.gate_seq;
  if (hipStreamWaitValue32(st, s.gate, v, hipStreamWaitValueEq, 0xFFFFFFFFu) != hipSuccess) {
    (void)hipGetLastError();                             // a runtime that reports the capability but refuses the call: this handle goes on without the gate
    h->gate_stage_b = false;
    return JN_OK;
  }
  gate.word = s.gate; gate.value = v; gate.info = s.h_info; gate.n = n; gate.st = st;
  return queue_stage_b(a, StageBInput{list_cap + HostWorker::kCornerPoints, h->tri_cap, true, s.h_payload, 0, true, false});
}

// The pool's work between the two GPU stages: the triangulations of the list the device filters wrote, or filters, list and
// triangulations from the candidates.  Fills FrameInfo and the payload in pinned memory, and the caller's status; returns what stage B
// takes from it (the frames packed back to back: one H2D copy per batch) and, in *ms, how long it took.
StageBInput Batch::host_stage(const StageA& a, float* ms) const {
  StageBInput r = {};
  const auto t0 = std::chrono::steady_clock::now();
  if (a.filtered) {
    // the counts are known, so the frames can be placed at once and the batch is one flat set of frame-side tasks
    int batch_most = 0;
    for (int i = 0; i < n; i++) batch_most = std::max(batch_most, (int)s.h_cnt[i]);
    note_support_counts(s, batch_most);
    for (int i = 0; i < n; i++) {
      FrameInfo& fi = s.h_info[i];
      memset(&fi, 0, sizeof(fi));
      fi.nsup = std::min(s.h_cnt[i], list_cap) + (h->hp.add_corners ? HostWorker::kCornerPoints : 0);   // elas.cpp:435
      fi.ok = fi.nsup >= 3;                              // elas.cpp:66-71
      r.payload_bytes += HostWorker::place(&fi, r.payload_bytes);
    }
    // Idle pool threads (a lone pair, a few large frames) are put to work inside the triangulations: every frame side
    // is cut into 2 or 4 independent parts (delaunay.h), three short pool rounds instead of one long one.
    const int want_parts = delaunay_parts(h, n);
    if (want_parts == 1) {
      h->pool->run(2 * n, [&](HostWorker& w, int k) {
        const int i = k >> 1;
        const uint16_t* arr = (a.arranged && s.h_arr_ok[k]) ? s.h_arr + (size_t)k * h->arr_stride : nullptr;
        w.triangulate_side_from_list(k & 1, s.h_list + (size_t)i * list_cap * 3, s.h_payload, &s.h_info[i], arr);
      });
    } else {
      h->pool->run(2 * n, [&](HostWorker& w, int k) {
        const int i = k >> 1;
        w.side_prepare(k & 1, s.h_list + (size_t)i * list_cap * 3, s.h_payload, &s.h_info[i], &s.sides[k], want_parts);
      });
      h->pool->run(2 * n * want_parts, [&](HostWorker&, int k) {
        HostWorker::SideState& st = s.sides[k / want_parts];
        if (k % want_parts < st.parts) st.dt.subtree(k % want_parts);
      });
      h->pool->run(2 * n, [&](HostWorker&, int k) { HostWorker::side_finish(k & 1, s.h_payload, &s.h_info[k >> 1], &s.sides[k]); });
    }
  } else {
    h->pool->run(n, [&](HostWorker& w, int i) {          // phase 1: filters + support list, per frame
      w.filter_and_list(s.h_can + (size_t)i * dp.cw * dp.ch, &s.h_info[i], &s.scratch[i], false);
    });
    for (int i = 0; i < n; i++) r.payload_bytes += HostWorker::place(&s.h_info[i], r.payload_bytes);
    h->pool->run(2 * n, [&](HostWorker& w, int k) {      // phase 2: one triangulation per frame and side
      const int i = k >> 1;
      w.triangulate_side(k & 1, s.scratch[i], s.h_payload, &s.h_info[i]);
    });
  }
  *ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int i = 0; i < n; i++) {
    const FrameInfo& fi = s.h_info[i];
    if (j.status) j.status[i] = fi.ok ? JN_OK : JN_ERR_FEW_SUPPORT;
    if (!fi.ok) continue;
    r.any_ok = true;
    r.max_tri = std::max(r.max_tri, std::max(fi.ntri[0], fi.ntri[1]));
    r.max_sup = std::max(r.max_sup, fi.nsup);
  }
  return r;
}

// The host route behind stage A: [stage B behind the gate ->] wait for stage A -> host stage -> stage B (or the gate opens) -> wait.
jn_status Batch::finish_host_route(const StageA& a, RouteResult* out) const {
  GateGuard gate;
  bool cleared = false;                                  // the two clears are on the stream already
  const jn_status gs = queue_gated_stage_b(a, gate, &cleared);
  if (gs != JN_OK) return gs;
  HIP_TRY(wait_event(s.ev[EV_D2H], h->wait_spin_us));
  StageBInput in = host_stage(a, &out->host_ms);
  out->any_ok = in.any_ok;
  if (gate.shut()) gate.open();
  else {
    // A latency-mode handle lets the two kernels that consume the payload read it where the host wrote it (pinned memory is visible to
    // the device): a lone pair's payload is ~50 KB read once, and the copy plus the pause behind it cost more than that (JN_ZERO_COPY=0/1).
    in.payload = h->zero_copy_payload ? s.h_payload : s.payload; in.cleared = cleared;
    const jn_status qs = queue_stage_b(a, in);
    if (qs != JN_OK) return qs;
  }
  HIP_TRY(wait_event(s.ev[EV_END], h->wait_spin_us));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

// One pass of the batch: stage A, then the route stage A settled on.  Returns with the batch complete on the GPU (or handed back).
jn_status run_route(jn_elas* h, Slot& s, const Job& j, bool force_host, RouteResult* out) {
  HIP_TRY(hipSetDevice(h->device));
  *out = RouteResult();
  out->t_begin = std::chrono::steady_clock::now();
  const Batch b = plan_batch(h, s, j, force_host);
  StageA a;
  const jn_status qs = b.queue_stage_a(&a);
  if (qs != JN_OK) return qs;
  return a.gpu_dt ? b.finish_gpu_route(a, out) : b.finish_host_route(a, out);
}

// The path's one exchange step (point_cloud.cpp:264-266 across rigs): the bins of this batch MIN-reduced over the ranks,
// as the batch's tail, issued by THIS worker (the submitting thread is not involved, the other slots keep the GPU busy).
// RCCL wants every rank to issue a communicator's collectives in one order: batches take their turn in submission order
// (every rank submits the same sequence), whatever order their host stages finished in.
// The scan is complete here (the route's last wait), so pack -> all-reduce -> unpack need no cross-stream dependency: chaining
// them to the slot's stream with events cost 0.66 ms per batch on a busy GPU (two queue hand-overs), this costs the
// kernels themselves plus one host wait (profiles/r03_merge_in_worker.txt).
// *host_ms: scan complete -> merged bins in place, on the worker's clock (its turn in the order included).
jn_status merge_tail(jn_elas* h, Slot& s, const Job& j, MergeTurn& turn, float* host_ms) {
  const auto t_m0 = std::chrono::steady_clock::now();
  jn_status ms_ = JN_OK;
  if (!h->test_slot_delay_us.empty()) {                  // tests only: this slot's host side takes longer, so batches reach their merge out of submission order
    size_t si = 0;
    while (si < h->slots.size() && h->slots[si].get() != &s) si++;
    const int us = h->test_slot_delay_us[si % h->test_slot_delay_us.size()];
    if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
  }
  {
    std::unique_lock<std::mutex> l(h->merge_m);
    h->merge_cv.wait(l, [&] { return h->merge_seq == j.seq; });
    ms_ = comm_merge_async(h->comm, j.n, j.sp.bins, j.dBins, j.dMeta, nullptr, s.ev_merged, s.d_flat);   // packed by k_scan_finish: all-reduce in place + unpack
    if (h->merge_log.size() >= 4096) h->merge_log.erase(h->merge_log.begin(), h->merge_log.begin() + 2048);
    h->merge_log.push_back(j.seq);
    h->merge_seq++;                                      // even on failure: the batches behind must not wait for ever
  }
  turn.done();
  h->merge_cv.notify_all();
  if (ms_ != JN_OK) return ms_;
  // a short wait (two small kernels): poll tightly, a sleep's granularity would show.  Bounded: a peer that died or never issued its
  // collective must not hang this rank — the communicator is aborted and this and all later scan batches return JN_ERR_COMM.
  const hipError_t we = wait_event(s.ev_merged, std::max(h->wait_spin_us, 400), h->comm_timeout_ms);
  if (we == hipErrorNotReady) { comm_abort(h->comm); return JN_ERR_COMM; }
  HIP_TRY(we);
  // another slot's merge timed out and aborted the communicator meanwhile: this merge's event completed because the aborted kernels
  // exited, its bins were never reduced
  if (comm_dead(h->comm)) return JN_ERR_COMM;
  *host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_m0).count();
  return JN_OK;
}

// The slot's record of the batch: jn_elas_last_times, _kernel_time, _merge_time, _bin_stats.
void read_stage_times(const jn_elas* h, Slot& s, int n, const RouteResult& r, float merge_ms) {
  const auto t_end = std::chrono::steady_clock::now();
  const bool stage_events = h->stage_events;
  auto ms = [&](int a, int b) { float v = 0; if (stage_events) hipEventElapsedTime(&v, s.ev[a], s.ev[b]); return v; };
  jn_stage_times& t = s.times;
  t.gpu_descriptor = ms(EV_BEGIN, EV_DESC); t.gpu_support = ms(EV_DESC, EV_SUPPORT); t.d2h = ms(EV_SUPPORT, EV_D2H);
  t.host_stage = r.host_ms;
  t.h2d = ms(EV_H2D0, EV_H2D);
  t.gpu_matching = ms(EV_H2D, EV_DENSE); t.gpu_lr = ms(EV_DENSE, EV_LR); t.gpu_speckle = ms(EV_LR, EV_SPECKLE);
  t.gpu_gap = ms(EV_SPECKLE, EV_GAP); t.gpu_adaptive_mean = ms(EV_GAP, EV_AM);
  t.total = std::chrono::duration<float, std::milli>(t_end - r.t_begin).count();
  s.last_n = n;
  s.dense_launches = r.any_ok && stage_events ? 1 : 0;
  if (s.dense_launches && h->plane_flow) {                   // k_bin | k_owner | k_dense_row: the matcher proper is timed from behind k_owner
    float a = 0, b = 0;
    hipEventElapsedTime(&a, s.ev[EV_RASTER], s.ev_owner); hipEventElapsedTime(&b, s.ev_owner, s.ev[EV_DENSE]);
    s.owner_ms = a; s.dense_ms = b;
  } else { s.dense_ms = ms(EV_RASTER, EV_DENSE); s.owner_ms = 0; }
  s.merge_ms = merge_ms;
}

// One batch on its slot's worker: GPU route -> (handed back ->) host route -> cross-rank merge -> stage times.
jn_status run_batch(jn_elas* h, Slot& s, const Job& j) {
  MergeTurn turn(h, j);
  if (j.merge && h->test_fail_seq >= 0 && (long long)j.seq == h->test_fail_seq) return JN_ERR_INTERNAL;
  RouteResult r;
  jn_status e = run_route(h, s, j, false, &r);
  if (e == JN_OK && r.handed_back) {                     // the whole batch again, host stage and all
    s.gpu_dt_fallbacks++;
    e = run_route(h, s, j, true, &r);
  }
  if (e != JN_OK) return e;
  float merge_ms = 0.f;
  if (j.merge) {
    e = merge_tail(h, s, j, turn, &merge_ms);
    if (e != JN_OK) return e;
  }
  read_stage_times(h, s, j.n, r, merge_ms);
  return JN_OK;
}

// Host pointers: images in (one copy per image when the caller's rows are padded or the images are apart, else one per
// side), the batch, the maps of the pairs that matched out (elas.cpp:66-71: a pair with too few support points leaves the
// caller's D1 / D2 untouched).  Runs on the slot's worker thread, so the copies of one slot overlap the kernels of the others.
jn_status run_batch_host(jn_elas* h, Slot& s, const Job& j) {
  HIP_TRY(hipSetDevice(h->device));
  const size_t px = (size_t)h->W * h->H, B = (size_t)h->max_batch;
  if (!s.st_img || !s.st_D) {                            // both or neither: a failed second allocation must not leave a half-made pair
    if (s.st_img) { hipFree(s.st_img); s.st_img = nullptr; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&s.st_img), 2 * B * px));
    if (hipMalloc(reinterpret_cast<void**>(&s.st_D), 2 * B * px * sizeof(float)) != hipSuccess) {
      hipFree(s.st_img); s.st_img = nullptr; s.st_D = nullptr;
      return JN_ERR_NO_DEVICE;
    }
  }
  hipStream_t st = s.stream;
  const uint8_t* src[2] = {j.hI1, j.hI2};
  for (int side = 0; side < 2; side++) {
    uint8_t* dst = s.st_img + side * B * px;
    if (j.pitch == h->W && j.stride == (int64_t)px) HIP_TRY(hipMemcpyAsync(dst, src[side], (size_t)j.n * px, hipMemcpyHostToDevice, st));
    else
      for (int b = 0; b < j.n; b++)
        HIP_TRY(hipMemcpy2DAsync(dst + b * px, h->W, src[side] + (size_t)b * j.stride, j.pitch, h->W, h->H, hipMemcpyHostToDevice, st));
  }
  std::vector<int32_t> local(j.n, JN_OK);
  Job d = j;
  d.host = false; d.staged = true; d.dI1 = s.st_img; d.dI2 = s.st_img + B * px; d.pitch = h->W; d.stride = (int64_t)px;
  const size_t opx = h->sub ? (size_t)(h->W / 2) * (h->H / 2) : px;          // pixels of an output map
  d.dD1 = s.st_D; d.dD2 = s.st_D + B * px; d.status = local.data();
  const jn_status r = run_batch(h, s, d);                 // stream-ordered behind the copies; synchronises at its end
  if (r != JN_OK) return r;
  for (int b = 0; b < j.n;) {                             // runs of matched pairs go out together
    if (local[b] != JN_OK) { b++; continue; }
    int e = b;
    while (e < j.n && local[e] == JN_OK) e++;
    HIP_TRY(hipMemcpyAsync(j.hD1 + b * opx, s.st_D + b * opx, (size_t)(e - b) * opx * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(j.hD2 + b * opx, s.st_D + B * px + b * opx, (size_t)(e - b) * opx * sizeof(float), hipMemcpyDeviceToHost, st));
    b = e;
  }
  HIP_TRY(hipEventRecord(s.ev[EV_END], st));
  HIP_TRY(wait_event(s.ev[EV_END], h->wait_spin_us));
  if (j.status) for (int b = 0; b < j.n; b++) j.status[b] = local[b];
  return JN_OK;
}

}  // namespace

void jnav::slot_loop(jn_elas* h, Slot* s) {
  pthread_setname_np(pthread_self(), "jn-slot");
  prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0);                 // the short sleeps of wait_event mean what they say (default slack: 50 us)
  hipSetDevice(h->device);
  for (;;) {
    Job j;
    {
      std::unique_lock<std::mutex> l(s->m);
      s->cv.wait(l, [s] { return s->quit || s->has_job; });
      if (s->quit) return;
      j = s->job; s->has_job = false;
    }
    const jn_status r = j.host ? run_batch_host(h, *s, j) : run_batch(h, *s, j);
    {
      std::lock_guard<std::mutex> l(s->m);
      s->result = r; s->busy = false;
    }
    s->cv.notify_all();
  }
}

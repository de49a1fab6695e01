// elas_handle.h — the jn_elas handle, its slots and their jobs, for the two files that make up the ELAS batch path: elas_batch.cpp (what a
// slot's worker does with a batch) and elas_api.cpp (the C entry points of include/jn_stereo.h that create the handle and feed its slots).
// Product code.
//
// One "slot" = one HIP stream + its buffers + one worker thread; several slots in flight overlap one batch's host stage with another
// batch's GPU stages.  elas_api.cpp writes a slot's Job under the slot's lock, elas_batch.cpp's slot_loop takes it from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "../../include/jn_stereo.h"
#include "kernels.h"
#include "dev_owner.h"
#include "nav_tail.h"
#include "host_stage.h"
#include "pool.h"

namespace jnav {

struct __attribute__((visibility("hidden"))) Job {
  int n = 0; const uint8_t* dI1 = nullptr; const uint8_t* dI2 = nullptr; int pitch = 0; int64_t stride = 0;
  float* dD1 = nullptr; float* dD2 = nullptr; int32_t* status = nullptr;
  // host-pointer form (jn_elas_submit_host): the worker stages the images in and the maps out around the batch
  uint64_t seq = 0; bool merge = false;                       // scan batch whose bins are MIN-reduced across ranks before it completes
  bool staged = false;                                        // the images were written on the slot's ordinary stream (run_batch_host): stage A stays there
  bool host = false; const uint8_t* hI1 = nullptr; const uint8_t* hI2 = nullptr; float* hD1 = nullptr; float* hD2 = nullptr;
  // optional tail of the node on the same stream (jn_elas_submit_scan): u8 map + LUT scan of D1
  bool scan = false; jn_scan_params sp = {}; const uint8_t* dLut = nullptr; uint8_t* dDispU8 = nullptr; double* dBins = nullptr; double* dMeta = nullptr;
  NavTails tails;                                             // what was attached to the slot when the scan batch was submitted
};

enum { EV_BEGIN, EV_DESC, EV_SUPPORT, EV_D2H, EV_H2D0, EV_H2D, EV_RASTER, EV_DENSE, EV_LR, EV_SPECKLE, EV_GAP, EV_AM, EV_END, EV_COUNT };

struct __attribute__((visibility("hidden"))) Slot {
  // Everything jn_elas_create makes for the slot is recorded here and released by jn_elas_destroy in one call.  What is made later keeps
  // its own release: st_img / st_D (run_batch_host frees a half-made pair itself) and the tails' scratch (NavTails::release).
  DevOwner own;
  hipStream_t stream = nullptr;
  hipEvent_t ev_merged = nullptr;                              // behind the cross-rig merge (created with the slot)
  hipEvent_t ev_head = nullptr;                                // behind the heavy head of stage A (descriptors + support matches): start-up pacing
  float merge_ms = 0.f;
  double* d_flat = nullptr;                                   // the merge's packed buffer of this slot [max_batch][1024 + 4] (written by k_scan_finish)
  hipStream_t stream_a = nullptr;                             // highest-priority stream for stage A (see Batch); only with JN_STAGE_A_PRIORITY=1
  uint32_t* gate = nullptr; uint32_t gate_seq = 0;            // latency mode: the word stage B's queued launches wait on (hipMallocSignalMemory), see GateGuard
  hipEvent_t ev[EV_COUNT] = {};
  // device
  uint4* desc = nullptr; uint8_t* planes = nullptr; int16_t* d_can = nullptr;   // descriptors: materialised (the old flow) OR the two Sobel planes (h->plane_flow)
  FrameInfo* info = nullptr; uint8_t* payload = nullptr; int32_t* bin_count = nullptr; BinEntry* bin_list = nullptr; int16_t* raw = nullptr;
  float* tmp = nullptr; int32_t* label = nullptr; int32_t* size = nullptr;
  uint32_t* mark = nullptr; uint32_t* gridbits = nullptr; TriRec* recs = nullptr;
  unsigned long long* scan_scratch = nullptr;                 // extrema of the scan tail, 4 per frame
  NavTails tails;                                             // attached costmap and sub-pixel tail, with their scratch (allocated by the attach calls)
  uint8_t* st_img = nullptr; float* st_D = nullptr;           // device staging of jn_elas_submit_host: [2][max_batch] images / maps, allocated on first use
  std::vector<FrameScratch> scratch;
  std::vector<HostWorker::SideState> sides;                  // [2 * max_batch]: per frame side, for the phased (parallel) triangulation
  // pinned host
  int16_t* h_can = nullptr; FrameInfo* h_info = nullptr; uint8_t* h_payload = nullptr;
  int16_t* h_list = nullptr; int32_t* h_cnt = nullptr;       // support lists the GPU writes straight into pinned memory
  uint16_t* h_arr = nullptr; int32_t* h_arr_ok = nullptr;    // alternating-cut arrangements per frame side (k_arrange), same route
  // the same four buffers in DEVICE memory, for handles that triangulate on the GPU: k_arrange and k_delaunay then read the list and the
  // arrangement from HBM instead of pulling ~26 KB per frame side over PCIe at the start of two latency-bound kernels
  int16_t* d_list = nullptr; int32_t* d_cnt = nullptr; uint16_t* d_arr = nullptr; int32_t* d_arr_ok = nullptr;
  uint8_t* dt_scratch = nullptr;                              // frames whose sides exceed one workgroup's LDS (1920x1080): the global structure of k_delaunay_sub / _top
  int arr_hint = 0;                                           // most support points a frame of this slot's last kArrHist batches had
  static constexpr int kArrHist = 4;
  int arr_hist[kArrHist] = {0, 0, 0, 0}; int arr_pos = 0;
  void* arr_scratch = nullptr;                                // device: working arrays of k_arrange for sides beyond its LDS capacity
  // worker
  std::thread th; std::mutex m; std::condition_variable cv;
  bool has_job = false, busy = false, quit = false;
  Job job; jn_status result = JN_OK;
  jn_stage_times times = {};
  float dense_ms = 0, owner_ms = 0; int dense_launches = 0;
  int last_n = 0;                                              // frames of the slot's last batch (jn_elas_bin_stats)
  int32_t* need_host = nullptr; int32_t* h_need = nullptr;     // per frame: sides k_delaunay handed back (device / pinned copy)
  long long gpu_dt_fallbacks = 0;                              // batches that went through the host stage after all
  hipEvent_t ev_owner = nullptr;                               // between k_owner and k_dense_row (plane flow, stage events on)
};

}  // namespace jnav

struct jn_elas {
  jn_elas_params p;
  jnav::DevParams dp;
  jnav::HostParams hp;
  int W = 0, H = 0, max_batch = 0, device = 0;
  size_t payload_cap = 0;
  int tri_cap = 0;
  // Where the support filters run.  The wavefront kernel is a serial chain of ~6*cw steps on one workgroup per
  // frame, so its duration does not depend on the batch size; the host filters take one pool round per
  // `threads` frames.  The device wins once a batch needs more than one round (and it frees the pool for Delaunay);
  // for a lone pair or a batch the pool swallows at once the host is quicker.  JN_HOST_FILTERS at create time:
  // unset = device when the classify + resolve kernels apply (no serial sweep; lattice and codes fit the LDS) or the
  // batch exceeds the pool size, "1" = always host, "0" = always device.  The host also takes over when no kernel can
  // take the lattice.
  int filter_min_batch = 4;
  int wait_spin_us = 60;            // JN_WAIT_SPIN_US; 1000 for max_batch == 1 (see wait_event)
  bool stage_events = true;         // JN_STAGE_EVENTS: default on, off for max_batch == 1 (see Batch)
  bool gpu_arrange = true;          // JN_GPU_ARRANGE=0: the host computes the alternating-cut arrangement itself (A/B, tests)
  int arr_cap = 0, arr_stride = 0;  // vertices per frame side k_arrange orders in LDS / at all (more: in global scratch / on the host)
  int dt_gcap = 0;                  // GPU triangulation: vertices per side beyond one workgroup's LDS that the global scratch lets through (0: none)
  bool split_delaunay = true;       // JN_SPLIT_DELAUNAY=0 keeps one task per frame side whatever the pool size (A/B, tests)
  bool filters_fast = false;        // the classify + resolve kernels apply (short, no serial sweep): device route for any batch size
  // cross-rig merge as the tail of a scan batch (jn_elas_set_comm): merges are queued in submission order on every rank
  jn_comm* comm = nullptr;
  std::mutex merge_m; std::condition_variable merge_cv;
  // Start-up pacing (JN_PACE, default on for batch handles).  After a synchronisation several batches are submitted at once and their
  // descriptor / support kernels share the GPU: all of them reach their host stage late, and the GPU then idles while the pool works
  // through four host stages.  A batch's stage A therefore waits (on the device) until the batch submitted before it has finished its two
  // heavy kernels — the phase the pipeline settles into by itself.  In steady state that event is long complete: the wait is a no-op.
  std::mutex pace_m; hipEvent_t pace_prev = nullptr; bool pace = false;
  bool sub = false;                 // param.subsampling: half-size maps (elas.h:82, :160-162); dph = the post-processing's parameters at that size
  jnav::DevParams dph = {};
  bool zero_copy_payload = false;   // latency mode: stage B reads the host stage's output in pinned memory instead of a copy of it
  bool arrange_sorts = false;       // hooks build, JN_ARRANGE_SORTS=1: k_arrange's sort forms where its rank form would run (A/B, tests)
  bool gpu_delaunay = false;        // batch handles: the triangulations' hull recursion on the GPU too (delaunay_gpu.hip; JN_GPU_DELAUNAY=0/1), no host stage
  bool plane_flow = true;           // descriptors assembled from the Sobel planes inside the matching kernels (JN_DESC_FLOW=desc: materialised, the old flow)
  std::atomic<bool> gate_stage_b{false};   // latency mode: stage B is queued behind a gate while the GPU runs stage A (JN_GATE_STAGE_B=0/1), see GateGuard
  uint64_t submit_seq = 0, merge_seq = 0;                     // next number handed to a scan batch / next batch allowed to queue its merge
  std::vector<uint64_t> merge_log;                            // submission numbers in the order their merges were queued (the last 4096; jn_elas_merge_order)
  int comm_timeout_ms = 30000;                                // JN_COMM_TIMEOUT_MS: a merge not complete by then is aborted (0: wait for ever)
  long long test_fail_seq = -1;                               // JN_TEST_FAIL_SEQ=k: the scan batch with submission number k fails before its kernels (tests: a rank's batch dies, the merge order must survive)
  std::vector<int> test_slot_delay_us;                        // JN_TEST_SLOT_DELAY_US="a,b,c,d": slot i's batches pause that long before their merge turn (tests: host stages of unequal length)
  std::unique_ptr<jnav::Pool> pool;
  std::vector<std::unique_ptr<jnav::Slot>> slots;
  // staging for the host-pointer drop-in call
  uint8_t* s_img = nullptr; float* s_D = nullptr; int s_pitch = 0;
  std::mutex api_m;
};

namespace jnav {

// elas_batch.cpp: the body of a slot's worker thread.  Takes the slot's jobs until the slot is told to quit.
__attribute__((visibility("hidden"))) void slot_loop(jn_elas* h, Slot* s);

// comm.cpp: the cross-rig merge, as the handle uses it
jn_status comm_merge_async(jn_comm* c, int n, int bins, double* dBins, double* dMeta, hipEvent_t ready, hipEvent_t done, double* packed);
jn_status comm_merge_identity(jn_comm* c, int n, int bins);
void comm_abort(jn_comm* c);
bool comm_dead(const jn_comm* c);
int comm_device(const jn_comm* c);

}  // namespace jnav

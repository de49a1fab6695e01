// elas_api.cpp — the C entry points of the ELAS handle (include/jn_stereo.h): create and destroy, the three submits, the attaches, wait,
// the synchronous calls and the slot's statistics.  Product code.
//
// The handle and its slots are elas_handle.h's; what a slot's worker does with a submitted batch is elas_batch.cpp's.
#include "elas_handle.h"
#include "hooks.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <sched.h>

using namespace jnav;

namespace {

// CPUs this process may really use: its affinity mask, cut down to the container's CPU quota (cgroup v2 cpu.max) — a pool
// sized by the machine's core count inside a container with a smaller quota gets the whole container throttled.
int usable_cpus() {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    long long quota = 0, period = 0;
    if (fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) n = std::min<long long>(n, std::max<long long>(1, quota / period));
    fclose(f);
  }
  return n;
}

int prior_radius(const jn_elas_params* p) { return (int)std::max((float)std::ceil(p->sigma * p->sradius), 2.0f); }   // elas.cpp:806

// jn_elas_create, step 1: what (p, W, H) alone decide — the kernels' and the host stage's parameters and the capacities that follow from
// them.  Touches no device.  JN_ERR_UNSUPPORTED: priors beyond the dense matcher's keys.
jn_status derive_params(jn_elas* h, const jn_elas_params* p, int W, int H) {
  const int radius = prior_radius(p);
  h->p = *p; h->W = W; h->H = H;
  DevParams& dp = h->dp;
  memset(&dp, 0, sizeof(dp));
  dp.W = W; dp.H = H; dp.pitch = (W + 63) / 64 * 64;
  dp.disp_max = p->disp_max; dp.disp_min = std::max(p->disp_min, 0); dp.support_texture = p->support_texture; dp.step = p->candidate_stepsize;
  h->sub = p->subsampling != 0;
  if (h->sub) dp.step += dp.step % 2;                                                    // elas.cpp:379-381: only even lines hold descriptors at half resolution
  dp.lr_threshold = p->lr_threshold; dp.support_threshold = p->support_threshold;
  dp.cw = (W + dp.step - 1) / dp.step; dp.ch = (H + dp.step - 1) / dp.step;            // elas.cpp:384-387
  dp.grid_size = p->grid_size;
  dp.grid_magic = p->grid_size > 1 ? (uint32_t)((1ull << 32) / (uint64_t)p->grid_size) + 1u : 0u;   // grid_size 1: kernels divide
  dp.gw = (int)std::ceil((float)W / (float)p->grid_size); dp.gh = (int)std::ceil((float)H / (float)p->grid_size);   // elas.cpp:90-91
  dp.match_texture = p->match_texture; dp.radius = radius;
  const float two_sigma_sq = 2 * p->sigma * p->sigma;
  for (int dd = 0; dd <= radius; dd++)                                                    // elas.cpp:802-805 (float math)
    dp.P[dd] = (int32_t)((-std::log(p->gamma + std::exp(-dd * dd / two_sigma_sq)) + std::log(p->gamma)) / p->beta);
  for (int dd = 0; dd <= radius; dd++)            // k_dense packs cost + prior into 24 bits of a key (bias 2^20)
    if (dp.P[dd] <= -(1 << 19) || dp.P[dd] >= (1 << 19)) return JN_ERR_UNSUPPORTED;
  dp.speckle_sim = p->speckle_sim_threshold; dp.speckle_size = p->speckle_size; dp.gap_width = p->ipol_gap_width;
  dp.add_corners = p->add_corners ? 1 : 0;
  if (h->sub) {                                         // the half-size maps' post-processing (elas.cpp:987-992, :1107-1112, :1292-1297, :1499-1504)
    h->dph = dp;
    h->dph.W = W / 2; h->dph.H = H / 2; h->dph.pitch = (W / 2 + 63) / 64 * 64;
    h->dph.speckle_size = (int32_t)(std::sqrt((float)p->speckle_size) * 2);
    h->dph.gap_width = p->ipol_gap_width / 2 + 1;
  }

  HostParams& hp = h->hp;
  hp.W = W; hp.H = H; hp.disp_max = p->disp_max; hp.step = dp.step; hp.incon_window_size = p->incon_window_size;
  hp.incon_threshold = p->incon_threshold; hp.incon_min_support = p->incon_min_support;
  hp.grid_size = p->grid_size; hp.gw = dp.gw; hp.gh = dp.gh; hp.cw = dp.cw; hp.ch = dp.ch;
  hp.add_corners = dp.add_corners;
  h->payload_cap = (HostWorker::payload_capacity(hp) + 255) / 256 * 256;
  h->tri_cap = 2 * (dp.cw * dp.ch + HostWorker::kCornerPoints) + 8;
  return JN_OK;
}

// jn_elas_create, step 2: the routes the handle's batches will take and every environment switch it reads, once, here: the pool, where the
// support filters run, the descriptors' data flow, the arrangement's capacities, where the triangulations run, pacing, zero copy, stage
// events, the gate.  Makes the host pool; of the device it asks one attribute (the gate's) and allocates nothing on it.
void decide_routes(jn_elas* h, int host_threads, int slots) {
  const jn_elas_params* p = &h->p;
  const DevParams& dp = h->dp;
  const HostParams& hp = h->hp;
  const int W = h->W, H = h->H, max_batch = h->max_batch, device = h->device;
  int nthreads = host_threads > 0 ? host_threads : usable_cpus();
  if (nthreads < 1) nthreads = 1;
  nthreads = std::min(nthreads, std::max(1, 8 * max_batch * slots));   // up to 2 sides x 4 parts per frame can run at once
  // latency-mode handles keep the pool threads that have just worked polling for 300 us (a lone pair's host stage is two 60 us tasks):
  // lone 640x480 pair 0.40 -> 0.35 ms.  (Running a synchronous call on the caller's thread instead of slot 0's worker was measured too: no gain.)
  int pool_spin = max_batch == 1 ? 300 : 0;
  if (const char* e = getenv("JN_POOL_SPIN_US")) pool_spin = atoi(e);
  h->pool.reset(new Pool(nthreads, hp, pool_spin));
  h->filter_min_batch = nthreads + 1;
  h->filters_fast = support_filters_fast(h->dp, p->incon_window_size, p->incon_min_support);
  // The plane data flow needs the LDS-staged forms of the two matching kernels; the parameter sets those do not take (support windows
  // beyond 2560 columns, grids below 8 pixels, priors beyond the keys' cost field) keep materialised descriptors and the kernels that read them.
  {
    const DescSrc probe{nullptr, 0, true};
    h->plane_flow = launch_support(nullptr, h->dp, max_batch, probe, nullptr, true) &&
                    launch_dense(nullptr, h->dp, max_batch, nullptr, nullptr, 0, nullptr, nullptr, nullptr, probe, nullptr, true);
    if (const char* e = getenv("JN_DESC_FLOW")) h->plane_flow = h->plane_flow && strcmp(e, "desc") != 0;
  }
  if (const char* e = getenv("JN_HOST_FILTERS")) h->filter_min_batch = atoi(e) ? (1 << 30) : 1;
  if (const char* e = getenv("JN_SPLIT_DELAUNAY")) h->split_delaunay = atoi(e) != 0;
  h->arr_cap = std::min(dp.cw * dp.ch, 8192);
  // Host route: sides with more vertices than k_arrange's 64-bit-key LDS form orders (8192; a 1920x1080 side has 11 k) are arranged on the
  // host (JN_ARRANGE_GLOBAL=1 in the hooks build sends them through the kernel's larger forms instead).  The GPU route (below) always
  // arranges on the device: 12288 vertices with compact keys in LDS (0.64 ms a 1080p batch), up to 16384 on global scratch (1.7 ms).
  h->arr_stride = (JN_HOOK_ENV("JN_ARRANGE_GLOBAL") && atoi(JN_HOOK_ENV("JN_ARRANGE_GLOBAL"))) ? std::min(dp.cw * dp.ch, 16384) : h->arr_cap;
  if (const char* e = JN_HOOK_ENV("JN_ARRANGE_SORTS")) h->arrange_sorts = atoi(e) != 0;
  h->gpu_arrange = !h->hp.add_corners;                     // the six corner points join the list on the host
  if (const char* e = getenv("JN_GPU_ARRANGE")) h->gpu_arrange = h->gpu_arrange && atoi(e) != 0;
  // Batch handles triangulate on the GPU as well (a latency-mode handle keeps the host stage: two pool threads finish a 640x480 pair's
  // two sides in 65 us, the kernel's serial top merges take longer than that); needs the device filters' list and the device arrangement.
  // (the kernels' FP64 predicates are exact for coordinates in (-2048, 2048); wider or taller images take their integer form)
  const bool gpu_dt_possible = max_batch > 1 && h->gpu_arrange && h->filters_fast;
  // Which of the two is faster depends on the host cores this process has (profiles/r05_gpu_delaunay_ab.txt, one MI355X): the kernel's top
  // merges are one thread each walking a seam through LDS (0.8-0.9 ms a batch, 42 bytes per vertex of every side held in LDS meanwhile):
  // 19.6 k pairs/s whatever the cores (0.3 busy); the host stage gives 22.0 k with ~10 busy cores where the scheduler may spread 16
  // threads over a whole socket, but 18.3 k pinned to 16 cores, 16.3 k to 12, 12.7 k to 8, 6.9 k to 4.  So: the GPU route for a process
  // PINNED to 16 cores or fewer (what a rank of a multi-GPU job gets: parallel.pin_rank) or with a CPU quota below 14, the host route
  // otherwise; JN_GPU_DELAUNAY=0/1 decides otherwise.
  {
    cpu_set_t set;
    const int pinned = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
    // (an explicit host_threads below 14 says the same thing — the caller's share of a quota that several ranks divide, which no rank can
    // see from its own affinity mask or cpu.max: bench.py passes quota / world)
    // Frames of 1920x1080 and beyond take the GPU route whatever the cores: their 11 k-point sides keep 12.8-14.4 host cores busy for
    // 4.9-5.7 k pairs/s, the kernels give 5.3-5.6 k with none (profiles/r06_full_hd_routes.txt, two boxes).
    h->gpu_delaunay = gpu_dt_possible && (pinned <= 16 || usable_cpus() < 14 || (host_threads > 0 && host_threads < 14) || (long long)W * H >= 1920LL * 1080);
  }
  if (const char* e = getenv("JN_GPU_DELAUNAY")) h->gpu_delaunay = gpu_dt_possible && atoi(e) != 0;
  // Sides with more support points than one workgroup's LDS holds (a 1920x1080 side has ~11 k) go through k_delaunay_sub / k_delaunay_top and
  // a global scratch (round 6); their arrangement then comes from k_arrange's compact-key LDS form (up to 12288 vertices a side) or its
  // global-scratch form (up to 16384).
  if (h->gpu_delaunay && dp.cw * dp.ch > delaunay_gpu_capacity(152 * 1024)) {
    h->dt_gcap = std::min(dp.cw * dp.ch, delaunay_gpu_max_points());
    h->arr_stride = std::max(h->arr_stride, std::min(dp.cw * dp.ch, 16384));
  }
  h->stage_events = max_batch > 1;
  h->wait_spin_us = max_batch > 1 ? 60 : 1000;
  if (const char* e = getenv("JN_WAIT_SPIN_US")) h->wait_spin_us = atoi(e);
  if (const char* e = getenv("JN_COMM_TIMEOUT_MS")) h->comm_timeout_ms = atoi(e);
  if (const char* e = JN_HOOK_ENV("JN_TEST_FAIL_SEQ")) h->test_fail_seq = atoll(e);
  if (const char* e = JN_HOOK_ENV("JN_TEST_SLOT_DELAY_US")) {
    for (const char* q = e; *q;) { h->test_slot_delay_us.push_back(atoi(q)); while (*q && *q != ',') q++; if (*q == ',') q++; }
  }
  h->pace = max_batch > 1 && slots > 1;
  if (const char* e = getenv("JN_PACE")) h->pace = atoi(e) != 0;
  h->zero_copy_payload = max_batch == 1;
  if (const char* e = getenv("JN_ZERO_COPY")) h->zero_copy_payload = atoi(e) != 0;
  if (const char* e = getenv("JN_STAGE_EVENTS")) h->stage_events = atoi(e) != 0;
  {
    int can_wait = 0;
    (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, device);
    h->gate_stage_b = max_batch == 1 && can_wait;
    if (const char* e = getenv("JN_GATE_STAGE_B")) h->gate_stage_b = atoi(e) != 0 && can_wait;
  }
}

// jn_elas_create, step 3, once per slot: its streams, events and buffers, all recorded in the slot's DevOwner.  The slot belongs to the
// handle before anything is made for it: after a failure jn_elas_destroy releases what there is.
jn_status make_slot(jn_elas* h) {
  const DevParams& dp = h->dp;
  const int W = h->W, H = h->H;
  const size_t px = (size_t)W * H, B = (size_t)h->max_batch;
  h->slots.emplace_back(new Slot());         // owned by the handle from the start: a failure below frees it too
  Slot* s = h->slots.back().get();
  DevOwner& own = s->own;
  HIP_TRY(own.stream(&s->stream, hipStreamNonBlocking));
  // Measured (profiles/r03_stage_a_priority_ab.txt): with stage A prioritised the pipelined 720p bench LOSES 12 % (17.5 k
  // against 20.2 k pairs/s) — the descriptor and support kernels of one slot then push the other slots' dense kernels
  // aside, and the GPU, not the host stage, is what the pipeline waits for.  Opt-in only: JN_STAGE_A_PRIORITY=1.
  if (getenv("JN_STAGE_A_PRIORITY") && atoi(getenv("JN_STAGE_A_PRIORITY")) != 0) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
      HIP_TRY(own.stream(&s->stream_a, hipStreamNonBlocking, greatest));
  }
  // blocking-sync events: the slot worker sleeps while the GPU runs instead of spinning on a core that
  // the host stage (and, on a multi-GPU node, the other ranks) could use
  for (int e = 0; e < EV_COUNT; e++) HIP_TRY(own.event(&s->ev[e], hipEventBlockingSync));
  HIP_TRY(own.event(&s->ev_merged)); HIP_TRY(own.event(&s->ev_head, hipEventDisableTiming)); HIP_TRY(own.event(&s->ev_owner));
  HIP_TRY(own.alloc(&s->need_host, B)); HIP_TRY(own.pinned(&s->h_need, B));
  if (h->gate_stage_b) {                                   // no signal memory: the handle simply queues stage B after the host stage
    if (own.signal(&s->gate, 8) == hipSuccess) { s->gate[0] = 0; s->gate[1] = 0; }
    else (void)hipGetLastError();
  }
  if (h->plane_flow) HIP_TRY(own.alloc(&s->planes, plane_bytes(W, H, 2 * (int)B) + 64));
  else HIP_TRY(own.alloc(&s->desc, 2 * B * px));
  HIP_TRY(own.alloc(&s->d_can, B * dp.cw * dp.ch));
  HIP_TRY(own.alloc(&s->info, B)); HIP_TRY(own.alloc(&s->payload, B * h->payload_cap));
  const size_t tiles = (size_t)((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH);
  HIP_TRY(own.alloc(&s->bin_count, 2 * B * tiles)); HIP_TRY(own.alloc(&s->bin_list, 2 * B * tiles * kBinCap));
  HIP_TRY(own.alloc(&s->raw, 2 * B * px));
  HIP_TRY(own.alloc(&s->tmp, B * px)); HIP_TRY(own.alloc(&s->label, B * px)); HIP_TRY(own.alloc(&s->size, B * px));
  HIP_TRY(own.alloc(&s->scan_scratch, B * 4));
  HIP_TRY(own.alloc(&s->d_flat, B * (1024 + 4)));
  const size_t grid_words = 2 * B * dp.gw * dp.gh * kGridWords;
  HIP_TRY(own.alloc(&s->mark, grid_words)); HIP_TRY(own.alloc(&s->gridbits, grid_words));
  HIP_TRY(own.alloc(&s->recs, 2 * B * (size_t)h->tri_cap));
  s->scratch.resize(B);
  s->sides.resize(2 * B);
  HIP_TRY(own.pinned(&s->h_can, B * dp.cw * dp.ch)); HIP_TRY(own.pinned(&s->h_info, B)); HIP_TRY(own.pinned(&s->h_payload, B * h->payload_cap));
  HIP_TRY(own.pinned(&s->h_list, B * dp.cw * dp.ch * 3)); HIP_TRY(own.pinned(&s->h_cnt, B));
  HIP_TRY(own.pinned(&s->h_arr, B * 2 * (size_t)h->arr_stride));
  if (h->arr_stride > h->arr_cap) HIP_TRY(own.alloc_bytes(&s->arr_scratch, arrange_scratch_bytes((int)B, h->arr_stride)));
  HIP_TRY(own.pinned(&s->h_arr_ok, B * 2));
  if (h->gpu_delaunay) {
    HIP_TRY(own.alloc(&s->d_list, B * dp.cw * dp.ch * 3)); HIP_TRY(own.alloc(&s->d_cnt, B));
    HIP_TRY(own.alloc(&s->d_arr, B * 2 * (size_t)h->arr_stride)); HIP_TRY(own.alloc(&s->d_arr_ok, B * 2));
    HIP_TRY(hipMemset(s->payload, 0, B * h->payload_cap));
    HIP_TRY(hipStreamSynchronize(nullptr));             // hipMemset only queues the fill, and the slot's streams do not wait for the null stream: a late fill would wipe a payload
    if (h->dt_gcap) HIP_TRY(own.alloc(&s->dt_scratch, delaunay_gpu_scratch_bytes((int)B, h->dt_gcap)));      // (a side k_delaunay hands back leaves its part unwritten: never uninitialised memory)
  }
  return JN_OK;
}

// The slot of that number, or null: a null handle or a number outside the handle's slots.
Slot* slot_of(jn_elas* h, int32_t slot) { return h && slot >= 0 && slot < (int)h->slots.size() ? h->slots[slot].get() : nullptr; }

// The slot's lock, held from the moment no batch is in flight on the slot.
std::unique_lock<std::mutex> lock_idle(Slot& s) {
  std::unique_lock<std::mutex> l(s.m);
  s.cv.wait(l, [&] { return !s.busy; });
  return l;
}

// Hands the slot's worker its next batch: once the slot is idle, `fill` writes the job, under the slot's lock.
template <typename Fill>
void enqueue(Slot& s, Fill&& fill) {
  {
    const std::unique_lock<std::mutex> l = lock_idle(s);
    fill(s.job);
    s.has_job = true; s.busy = true;
  }
  s.cv.notify_all();
}

// what the three submits ask of a batch's images and maps, on the device or on the host
bool batch_ok(const jn_elas* h, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t pitch, int64_t image_stride, const float* D1, const float* D2) {
  return n >= 1 && n <= h->max_batch && I1 && I2 && D1 && D2 && pitch >= h->W &&
         (n == 1 || image_stride >= (int64_t)pitch * h->H);    // image b starts at base + b*image_stride: images must not overlap
}

}  // namespace

extern "C" {

void jn_elas_params_default(jn_elas_params* p, int32_t setting) {
  // elas.h:92-145
  p->disp_min = 0; p->disp_max = 255; p->support_texture = 10; p->candidate_stepsize = 5;
  p->incon_window_size = 5; p->incon_threshold = 5; p->incon_min_support = 5; p->grid_size = 20;
  p->beta = 0.02f; p->sigma = 1; p->lr_threshold = 2; p->speckle_sim_threshold = 1; p->speckle_size = 200;
  p->subsampling = 0;
  if (setting == JN_SETTING_ROBOTICS) {
    p->support_threshold = 0.85f; p->add_corners = 0; p->gamma = 3; p->sradius = 2; p->match_texture = 1;
    p->ipol_gap_width = 3; p->filter_median = 0; p->filter_adaptive_mean = 1; p->postprocess_only_left = 1;
  } else {
    p->support_threshold = 0.95f; p->add_corners = 1; p->gamma = 5; p->sradius = 3; p->match_texture = 0;
    p->ipol_gap_width = 5000; p->filter_median = 1; p->filter_adaptive_mean = 0; p->postprocess_only_left = 0;
  }
}

jn_status jn_elas_create(const jn_elas_params* p, int32_t W, int32_t H, int32_t max_batch, int32_t device,
                         int32_t host_threads, int32_t slots, jn_elas** out) {
  if (!p || !out || W < 32 || H < 32 || W > 8192 || H > 8192 || max_batch < 1 || slots < 1) return JN_ERR_INVALID;
  *out = nullptr;
  const int radius = prior_radius(p);
  if ((p->subsampling && ((W | H) & 1)) || p->disp_max > 255 || p->disp_max < 10 ||      // odd sizes with subsampling: the reference's half-size addressing runs over its rows
      p->disp_min > p->disp_max || p->ipol_gap_width < 0 || p->candidate_stepsize < 1 ||
      p->grid_size < 1 || radius > 7 || p->incon_window_size < 0)
    return JN_ERR_UNSUPPORTED;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return JN_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));

  // any failure from here on releases whatever was allocated so far (jn_elas_destroy tolerates null buffers and
  // workers that were never started)
  std::unique_ptr<jn_elas, void (*)(jn_elas*)> h(new jn_elas(), jn_elas_destroy);
  HIP_TRY(configure_device_kernels());
  h->max_batch = max_batch; h->device = device;
  const jn_status ds = derive_params(h.get(), p, W, H);
  if (ds != JN_OK) return ds;
  decide_routes(h.get(), host_threads, slots);
  for (int i = 0; i < slots; i++) {
    const jn_status ss = make_slot(h.get());
    if (ss != JN_OK) return ss;
  }
  h->s_pitch = h->dp.pitch;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->s_img), 2 * (size_t)H * h->dp.pitch));
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&h->s_D), 2 * (size_t)W * H * sizeof(float)));
  for (auto& s : h->slots) s->th = std::thread(slot_loop, h.get(), s.get());
  *out = h.release();
  return JN_OK;
}

void jn_elas_destroy(jn_elas* h) {
  if (!h) return;
  hipSetDevice(h->device);
  for (auto& s : h->slots) {
    { const std::unique_lock<std::mutex> l = lock_idle(*s); s->quit = true; }
    s->cv.notify_all();
    if (s->th.joinable()) s->th.join();
  }
  hipSetDevice(h->device);
  for (auto& s : h->slots) {
    hipFree(s->st_img); hipFree(s->st_D); s->tails.release();   // made after jn_elas_create: their own release (see Slot)
    s->own.release();
  }
  hipFree(h->s_img); hipFree(h->s_D);
  h->pool.reset();
  delete h;
}

jn_status jn_elas_submit(jn_elas* h, int32_t slot, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch,
                         int64_t image_stride, float* dD1, float* dD2, int32_t* status) {
  Slot* s = slot_of(h, slot);
  if (!s || !batch_ok(h, n, dI1, dI2, pitch, image_stride, dD1, dD2)) return JN_ERR_INVALID;
  enqueue(*s, [&](Job& j) { j = Job{n, dI1, dI2, pitch, image_stride, dD1, dD2, status}; });
  return JN_OK;
}

jn_status jn_elas_submit_host(jn_elas* h, int32_t slot, int32_t n, const uint8_t* I1, const uint8_t* I2, int32_t pitch,
                              int64_t image_stride, float* D1, float* D2, int32_t* status) {
  Slot* s = slot_of(h, slot);
  if (!s || !batch_ok(h, n, I1, I2, pitch, image_stride, D1, D2)) return JN_ERR_INVALID;
  enqueue(*s, [&](Job& j) {
    j = Job{};
    j.n = n; j.pitch = pitch; j.stride = image_stride; j.status = status;
    j.host = true; j.hI1 = I1; j.hI2 = I2; j.hD1 = D1; j.hD2 = D2;
  });
  return JN_OK;
}

jn_status jn_elas_submit_scan(jn_elas* h, int32_t slot, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch,
                              int64_t image_stride, float* dD1, float* dD2, const jn_scan_params* sp, const uint8_t* dLut,
                              uint8_t* dDispU8, double* dBins, double* dMeta, int32_t* status) {
  Slot* s = slot_of(h, slot);
  if (!s || !batch_ok(h, n, dI1, dI2, pitch, image_stride, dD1, dD2) || !sp || !dLut || !dDispU8 || !dBins || !dMeta || sp->bins < 1 || sp->bins > 1024)
    return JN_ERR_INVALID;
  if (h->sub) return JN_ERR_UNSUPPORTED;                  // the node's tail works on full-size maps (its Q matrix and LUT are the image's)
  enqueue(*s, [&](Job& j) {
    j = Job{n, dI1, dI2, pitch, image_stride, dD1, dD2, status};
    j.scan = true; j.sp = *sp; j.dLut = dLut; j.dDispU8 = dDispU8; j.dBins = dBins; j.dMeta = dMeta;
    j.tails = s->tails;
    std::lock_guard<std::mutex> g(h->merge_m);             // the submitting thread numbers the batches: same order on every rank
    if (h->comm) { j.merge = true; j.seq = h->submit_seq++; }
  });
  return JN_OK;
}

jn_status jn_elas_attach_costmap(jn_elas* h, int32_t slot, const jn_costmap_params* cp, uint16_t* dHits, int8_t* dGrid) {
  Slot* s = slot_of(h, slot);
  if (!s) return JN_ERR_INVALID;
  const std::unique_lock<std::mutex> l = lock_idle(*s);     // no batch in flight on the slot
  return s->tails.attach_costmap(h->device, h->max_batch, cp, dHits, dGrid);
}

jn_status jn_elas_attach_subpix(jn_elas* h, int32_t slot, const jn_costmap_params* cp, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid) {
  Slot* s = slot_of(h, slot);
  if (!s) return JN_ERR_INVALID;
  const std::unique_lock<std::mutex> l = lock_idle(*s);     // no batch in flight on the slot
  return s->tails.attach_subpix(h->device, h->max_batch, cp, dBins, dMeta, dHits, dGrid);
}

jn_status jn_elas_set_comm(jn_elas* h, jn_comm* c) {
  if (!h) return JN_ERR_INVALID;
  if (c && comm_device(c) != h->device) return JN_ERR_INVALID;
  for (auto& s : h->slots) lock_idle(*s);                   // no batch in flight
  std::lock_guard<std::mutex> g(h->merge_m);
  if (c && comm_dead(c)) return JN_ERR_COMM;
  h->comm = c; h->submit_seq = 0; h->merge_seq = 0; h->merge_log.clear();
  return JN_OK;
}

int32_t jn_elas_merge_order(jn_elas* h, uint64_t* out, int32_t cap) {
  if (!h || !out || cap < 1) return 0;
  std::lock_guard<std::mutex> g(h->merge_m);
  const size_t k = std::min<size_t>(h->merge_log.size(), (size_t)cap);
  std::copy(h->merge_log.end() - k, h->merge_log.end(), out);
  return (int32_t)k;
}

jn_status jn_elas_route_stats(jn_elas* h, int32_t slot, int32_t out[3]) {
  const Slot* s = slot_of(h, slot);
  if (!s || !out) return JN_ERR_INVALID;
  out[0] = h->gpu_delaunay ? 1 : 0; out[1] = (int32_t)s->gpu_dt_fallbacks; out[2] = h->plane_flow ? 1 : 0;
  return JN_OK;
}

jn_status jn_elas_bin_stats(jn_elas* h, int32_t slot, int32_t out[3]) {
  const Slot* sl = slot_of(h, slot);
  if (!sl || !out) return JN_ERR_INVALID;
  const Slot& s = *sl;
  out[0] = out[1] = out[2] = 0;
  if (s.last_n < 1) return JN_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t tiles = (size_t)((h->W + kTileW - 1) / kTileW) * ((h->H + kTileH - 1) / kTileH), count = (size_t)s.last_n * 2 * tiles;
  std::vector<int32_t> c(count);
  HIP_TRY(hipMemcpy(c.data(), s.bin_count, count * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int32_t x : c) { out[0] = std::max(out[0], x); out[1] += x > (int32_t)kBinLds; out[2] += x > (int32_t)kBinCap; }
  return JN_OK;
}

jn_status jn_elas_merge_time(jn_elas* h, int32_t slot, float* ms) {
  const Slot* s = slot_of(h, slot);
  if (!s || !ms) return JN_ERR_INVALID;
  *ms = s->merge_ms;
  return JN_OK;
}

jn_status jn_elas_wait(jn_elas* h, int32_t slot) {
  Slot* s = slot_of(h, slot);
  if (!s) return JN_ERR_INVALID;
  const std::unique_lock<std::mutex> l = lock_idle(*s);
  return s->result;
}

jn_status jn_elas_process_batch(jn_elas* h, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch,
                                int64_t image_stride, float* dD1, float* dD2, int32_t* status) {
  const jn_status r = jn_elas_submit(h, 0, n, dI1, dI2, pitch, image_stride, dD1, dD2, status);
  if (r != JN_OK) return r;
  return jn_elas_wait(h, 0);
}

jn_status jn_elas_process(jn_elas* h, const uint8_t* I1, const uint8_t* I2, float* D1, float* D2, const int32_t dims[3]) {
  if (!h || !I1 || !I2 || !D1 || !D2 || !dims) return JN_ERR_INVALID;
  if (dims[0] != h->W || dims[1] != h->H || dims[2] < dims[0]) return JN_ERR_INVALID;
  std::lock_guard<std::mutex> guard(h->api_m);
  HIP_TRY(hipSetDevice(h->device));
  const size_t img = (size_t)h->H * h->s_pitch, px = (size_t)h->W * h->H;
  HIP_TRY(hipMemcpy2D(h->s_img, h->s_pitch, I1, dims[2], h->W, h->H, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy2D(h->s_img + img, h->s_pitch, I2, dims[2], h->W, h->H, hipMemcpyHostToDevice));
  int32_t st = JN_OK;
  const jn_status r = jn_elas_process_batch(h, 1, h->s_img, h->s_img + img, h->s_pitch, 0, h->s_D, h->s_D + px, &st);
  if (r != JN_OK) return r;
  if (st != JN_OK) {                        // elas.cpp:66-71: message, outputs untouched
    printf("ERROR: Need at least 3 support points!\n");
    return (jn_status)st;
  }
  const size_t opx = h->sub ? (size_t)(h->W / 2) * (h->H / 2) : px;          // elas.h:160-162: half-size maps with subsampling
  HIP_TRY(hipMemcpy(D1, h->s_D, opx * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(D2, h->s_D + px, opx * sizeof(float), hipMemcpyDeviceToHost));
  return JN_OK;
}

jn_status jn_elas_last_times(jn_elas* h, int32_t slot, jn_stage_times* out) {
  const Slot* s = slot_of(h, slot);
  if (!s || !out) return JN_ERR_INVALID;
  *out = s->times;
  return JN_OK;
}

jn_status jn_elas_kernel_time(jn_elas* h, int32_t slot, const char* kernel, float* avg_ms, int32_t* launches) {
  const Slot* s = slot_of(h, slot);
  if (!s || !kernel || !avg_ms || !launches) return JN_ERR_INVALID;
  const std::string k(kernel);
  if (k == "k_dense" || k == "k_dense_row") *avg_ms = s->dense_ms;      // the dense matcher of this handle's data flow
  else if (k == "k_owner") *avg_ms = s->owner_ms;
  else return JN_ERR_INVALID;
  *launches = s->dense_launches;
  return JN_OK;
}

}  // extern "C"

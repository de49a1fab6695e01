// sgm.hip — the semi-global-matching mode (include/jn_sgm.h): its C ABI.  Product code.
//
// No reference counterpart (the reference's only matcher is libelas); the definition is in jn_sgm.h and its scalar
// restatement (the checker, test infrastructure only) lives outside the product.  Everything is integer arithmetic, so the bar is bit-exactness.
// The kernels are sgm_sweep.hip's four sweeps (lanes = pixels).  Round 2's one-wave-per-line kernels (lanes = disparities, eight u8 volumes,
// 16 W H D bytes of traffic, 1.3 k pairs/s) lived here behind JN_SGM_IMPL=0 until round 5; their description and numbers: DESIGN_HISTORY.md.
#include <hip/hip_runtime.h>
#include "hooks.h"
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../include/jn_sgm.h"
#include "../../include/jn_sgm_cost.h"
#include "../../include/jn_costmap.h"
#include "../../include/jn_subpix.h"
#include "../../include/jn_postfilter.h"
#include "sgm_sweep.h"
#include "bm_mfma.h"            // the block-SSD cost volume (jn_sgm_cost.h): the matrix-core pass with bytes in place of a winner
#include "census.h"             // the census / Hamming cost volume (jn_sgm_cost.h)
#include "dev_owner.h"
#include "nav_tail.h"           // kernels.h's launch_scan, and NavTails: the node's tails on a slot's stream (jn_sgm_submit_scan)

namespace {

__global__ void __launch_bounds__(256) k_sgm_to_u8(const int16_t* __restrict__ d, int subpixel, uint8_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int v = d[i];
  if (v < 0) { out[i] = 0; return; }
  if (subpixel) { const int q = v >> 4, r = v & 15; v = q + ((r > 8 || (r == 8 && (q & 1))) ? 1 : 0); }   // half to even
  out[i] = (uint8_t)min(v, 255);
}

}  // namespace

struct jn_sgm {
  jn_sgm_params p;
  int W = 0, H = 0, max_batch = 0, device = 0;
  jnav_sgm::SwDev sw = {};
  jnav_sgm::SweepSizes sizes = {};
  // include/jn_sgm_cost.h: where the costs of the sweeps come from.  SAD3 (jn_sgm_create): computed inside them; BLOCK_SSD: a slot's own
  // volume, written by bm_mfma.hip's producer ahead of the sweeps; CENSUS: the same with census.hip's producer; EXTERNAL: the caller's
  // volume (jn_sgm_aggregate_batch)
  jn_sgm_cost_params cost = {JN_SGM_COST_SAD3, 0, 0, 0};
  jnav_bmq::QDev bq = {};
  jnav_bmq::Sizes bqz = {};
  jnav_census::CDev cq = {};
  jnav_census::Sizes cqz = {};
  bool makes_volume() const { return cost.cost_function == JN_SGM_COST_BLOCK_SSD || cost.cost_function == JN_SGM_COST_CENSUS; }
  // One slot: its own sweep buffers, stream and events.  Slot 0 is made with the handle (jn_sgm_process_batch runs on it), the others the
  // first time they are used (jn_sgm_submit_scan / jn_sgm_wait).  Batches on different slots overlap on the GPU: the upward sweep's tail
  // (the last blocks of its parallelogram run alone) is filled by the next batch's horizontal and downward sweeps.
  // Everything below except the tails' scratch (NavTails::release) and the buffers' side stream (sweep_release) belongs to `own`.
  struct Slot {
    jnav::DevOwner own;
    jnav_sgm::SweepBuffers sb = {};
    uint8_t* cost = nullptr;                    // BLOCK_SSD, CENSUS: the slot's cost volume [max_batch][H][W][D] ...
    uint8_t* bg = nullptr;                      // ... BLOCK_SSD: the producer's prefiltered rows and patch norms (bm_mfma.h)
    int32_t* bQ = nullptr;
    void* csig = nullptr;                       // ... CENSUS: the signatures of both eyes (census.h)
    hipStream_t stream = nullptr;               // its own, or with JN_SGM_STREAMS a lower slot's (`shared`: not in `own`)
    hipEvent_t ev[4] = {};
    hipEvent_t ev_end = nullptr;                // recorded behind EVERYTHING a submit queued (sweeps + the scan tail); what jn_sgm_wait waits for
    unsigned long long* scan_scratch = nullptr; // [max_batch][4], the scan tail's extrema (made by the first scan batch)
    bool ready = false, shared = false, pending = false;
    jnav::NavTails tails;                       // what jn_sgm_attach_costmap / _subpix / _postfilter attached to the slot's scan batches
  };
  enum { kSgmSlots = 8 };
  Slot slots[kSgmSlots];
  jn_sgm_times times = {};                      // of the batch waited for last (jn_sgm_last_times)
  __attribute__((visibility("hidden"))) ~jn_sgm() = default;   // (not trivial any more; the library exports its C ABI only)
};

static jn_status sgm_make_slot(jn_sgm* h, int slot);

// What sgm_make_slot makes; a failure returns half-way and leaves the release to it.
static jn_status sgm_slot_resources(jn_sgm* h, int slot) {
  jn_sgm::Slot& s = h->slots[slot];
  const jnav_sgm::SweepSizes& z = h->sizes;
  if (h->cost.cost_function == JN_SGM_COST_SAD3) HIP_TRY(s.own.alloc(&s.sb.gm, z.gm));
  if (h->makes_volume()) HIP_TRY(s.own.alloc(&s.cost, (size_t)h->max_batch * h->W * h->H * h->sw.D));
  if (h->cost.cost_function == JN_SGM_COST_BLOCK_SSD) {
    HIP_TRY(s.own.alloc(&s.bg, h->bqz.g));
    HIP_TRY(s.own.alloc_bytes(reinterpret_cast<void**>(&s.bQ), h->bqz.q));
  }
  if (h->cost.cost_function == JN_SGM_COST_CENSUS) HIP_TRY(s.own.alloc_bytes(&s.csig, h->cqz.sig));
  HIP_TRY(s.own.alloc(&s.sb.volF, z.vol * (h->sw.wide ? 2 : 1)));
  HIP_TRY(s.own.alloc(&s.sb.volH0, z.vol));
  HIP_TRY(s.own.alloc(&s.sb.volH1, z.vol));
  HIP_TRY(s.own.alloc_bytes(reinterpret_cast<void**>(&s.sb.gx), z.gx));
  s.sb.gx_bytes = z.gx;
  if (slot != 0) s.sb.epoch = h->slots[0].sb.epoch;
  else if (const char* e = JN_HOOK_ENV("JN_SGM_EPOCH_START")) s.sb.epoch = (uint32_t)atoi(e) & 0xFFFFu;   // test hook: start next to the tag's wrap-around
  HIP_TRY(s.own.alloc_bytes(reinterpret_cast<void**>(&s.sb.flags), z.flags));
  HIP_TRY(s.own.alloc_bytes(reinterpret_cast<void**>(&s.sb.minr), z.minr));
  HIP_TRY(s.own.alloc_bytes(reinterpret_cast<void**>(&s.sb.dl), z.dl));
  static const int share = getenv("JN_SGM_STREAMS") ? atoi(getenv("JN_SGM_STREAMS")) : 0;     // experiment: slot s queues on the stream of slot s % share
  if (share > 0 && slot >= share) {
    const int lower = slot % share;
    const jn_status el = sgm_make_slot(h, lower);
    if (el != JN_OK) return el;
    s.stream = h->slots[lower].stream; s.shared = true;
  } else HIP_TRY(s.own.stream(&s.stream, hipStreamNonBlocking));
  // tag 0 = "never written" (sgm_sweep.hip, k_sw_w).  On the stream the sweeps run on, ahead of the slot's first sweep: hipMemset returns
  // once the fill is QUEUED on the null stream, which a non-blocking stream does not wait for — a fill that runs late wipes columns a
  // block is still waiting to read.
  HIP_TRY(hipMemsetAsync(s.sb.gx, 0, s.sb.gx_bytes, s.stream));
  for (auto& e : s.ev) HIP_TRY(s.own.event(&e));
  return JN_OK;
}

// A slot's buffers, stream and events, made once.  A slot that fails half-way gives back what it made and stays not ready.
static jn_status sgm_make_slot(jn_sgm* h, int slot) {
  jn_sgm::Slot& s = h->slots[slot];
  if (s.ready) return JN_OK;
  const jn_status e = sgm_slot_resources(h, slot);
  if (e != JN_OK) {
    s.own.release();
    s.sb = {}; s.stream = nullptr; s.shared = false;
    s.cost = nullptr; s.bg = nullptr; s.bQ = nullptr; s.csig = nullptr;
    for (auto& v : s.ev) v = nullptr;
    return e;
  }
  s.ready = true;
  return JN_OK;
}

// The stage times of the slot's last batch, once it is complete.
static void sgm_read_times(jn_sgm* h, const jn_sgm::Slot& s) {
  jn_sgm_times& t = h->times;
  hipEventElapsedTime(&t.prefilter, s.ev[0], s.ev[1]);
  hipEventElapsedTime(&t.paths, s.ev[1], s.ev[2]);
  hipEventElapsedTime(&t.wta, s.ev[2], s.ev[3]);
  hipEventElapsedTime(&t.total, s.ev[0], s.ev[3]);
}

// The cost volume of a BLOCK_SSD or CENSUS handle, queued on the slot's stream.
static hipError_t sgm_queue_volume(jn_sgm* h, jn_sgm::Slot& s, int n, const uint8_t* dI1, const uint8_t* dI2, int pitch, long long stride, uint8_t* cost) {
  if (h->cost.cost_function == JN_SGM_COST_CENSUS) return jnav_census::cost_volume(h->cq, n, dI1, dI2, pitch, stride, s.csig, h->cost.cost_max, cost, s.stream);
  return jnav_bmq::cost_volume(h->bq, n, dI1, dI2, pitch, stride, s.bg, s.bQ, h->cost.cost_shift, h->cost.cost_max, cost, s.stream);
}

// The whole mode of a slot's batch on its stream: the sweeps, behind the cost volume's producer on a BLOCK_SSD or CENSUS handle (ev[0] ..
// ev[1] then span the producer: jn_sgm_times.prefilter).
static hipError_t sgm_queue(jn_sgm* h, jn_sgm::Slot& s, int n, const uint8_t* dI1, const uint8_t* dI2, int pitch, long long stride, int16_t* dDisp,
                            bool side_overlap, bool lr_kernel) {
  if (h->cost.cost_function == JN_SGM_COST_SAD3) return jnav_sgm::sweep_run(h->sw, n, dI1, dI2, pitch, stride, dDisp, s.stream, s.sb, s.ev, side_overlap, lr_kernel);
  hipError_t e;
  if ((e = hipEventRecord(s.ev[0], s.stream)) != hipSuccess) return e;
  if ((e = sgm_queue_volume(h, s, n, dI1, dI2, pitch, stride, s.cost)) != hipSuccess) return e;
  return jnav_sgm::sweep_run_cost(h->sw, n, s.cost, dDisp, s.stream, s.sb, s.ev, side_overlap, lr_kernel);
}

// The frame of the synchronous calls: slot 0 idle, `queue` on its stream, wait, the stage times where the call spans the sweeps.
template <class Queue>
static jn_status sgm_run_sync(jn_sgm* h, bool read_times, Queue queue) {
  jn_sgm::Slot& s = h->slots[0];
  if (s.pending) return JN_ERR_INVALID;                         // slot 0's buffers carry a submitted batch: jn_sgm_wait(h, 0) first
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(queue(s));
  HIP_TRY(hipStreamSynchronize(s.stream));
  HIP_TRY(hipGetLastError());
  if (read_times) sgm_read_times(h, s);
  return JN_OK;
}

extern "C" {

void jn_sgm_params_default(jn_sgm_params* p) {
  p->num_disparities = 128; p->P1 = 10; p->P2 = 60; p->prefilter_cap = 31; p->lr_max_diff = 1; p->subpixel = 0;
}

void jn_sgm_destroy(jn_sgm* h) {
  if (!h) return;
  hipSetDevice(h->device);
  for (auto& s : h->slots) if (s.stream && !s.shared) hipStreamSynchronize(s.stream);   // (a shared stream: once, by the slot that made it)
  for (auto& s : h->slots) {
    jnav_sgm::sweep_release(s.sb);
    s.tails.release();
    s.own.release();
  }
  delete h;
}

void jn_sgm_cost_params_default(jn_sgm_cost_params* c) {
  c->cost_function = JN_SGM_COST_BLOCK_SSD; c->block_radius = 2; c->cost_shift = 5; c->cost_max = 127;
}

// Every handle is made here; jn_sgm_create is the SAD3 case.  Refusals in the ABI's order, all before any device call: INVALID, UNSUPPORTED, NO_DEVICE.
jn_status jn_sgm_create_cost(const jn_sgm_params* p, const jn_sgm_cost_params* c, int32_t W, int32_t H, int32_t max_batch, int32_t device, jn_sgm** out) {
  if (!p || !c || !out || W < 8 || H < 8 || W > 8192 || H > 8192 || max_batch < 1) return JN_ERR_INVALID;
  *out = nullptr;
  const int D = p->num_disparities, fn = c->cost_function;
  const bool sad3 = fn == JN_SGM_COST_SAD3, ssd = fn == JN_SGM_COST_BLOCK_SSD, census = fn == JN_SGM_COST_CENSUS;
  if (!sad3 && !ssd && !census && fn != JN_SGM_COST_EXTERNAL) return JN_ERR_UNSUPPORTED;
  if ((D != 64 && D != 128 && D != 256) || p->prefilter_cap < 1 || p->prefilter_cap > 31 || p->P1 < 0 || p->P2 < p->P1) return JN_ERR_UNSUPPORTED;
  // Every L_r <= max C + P2 must fit a byte (jn_sgm.h), side by side for the two kinds of cost:
  //   computed (SAD3)   max C = 6 cap:            6 cap + P2 <= 255
  //   a volume          max C = cost_max >= 1:    cost_max + P2 <= 255 where the handle makes the volume, and P2 <= 254 (room for a cost of 1) in
  //                     any case: an EXTERNAL volume's bytes <= 255 - P2 are the caller's word
  if (sad3 ? 6 * p->prefilter_cap + p->P2 > 255 : p->P2 > 254) return JN_ERR_UNSUPPORTED;
  if ((ssd || census) && (c->block_radius < 2 || c->block_radius > 4 || c->cost_max < 1 || c->cost_max + p->P2 > 255)) return JN_ERR_UNSUPPORTED;
  if (ssd && (c->cost_shift < 0 || c->cost_shift > 12)) return JN_ERR_UNSUPPORTED;   // (CENSUS: cost_shift is not used)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return JN_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  jn_sgm* h = new jn_sgm();
  h->p = *p; h->W = W; h->H = H; h->max_batch = max_batch; h->device = device;
  if (sad3) jnav_sgm::sweep_geometry(W, H, D, p->P1, p->P2, p->prefilter_cap, p->lr_max_diff, p->subpixel, &h->sw, &h->sizes, max_batch);
  else {
    h->cost = *c;
    jnav_sgm::sweep_geometry_cost(W, H, D, p->P1, p->P2, p->lr_max_diff, p->subpixel, &h->sw, &h->sizes, max_batch);
    h->sw.cap = p->prefilter_cap;
  }
  if (ssd) jnav_bmq::geometry(W, H, D, c->block_radius, p->prefilter_cap, p->lr_max_diff, p->subpixel, &h->bq, &h->bqz, max_batch);
  if (census) jnav_census::geometry(W, H, D, c->block_radius, &h->cq, &h->cqz, max_batch);
  const jn_status e = sgm_make_slot(h, 0);
  if (e != JN_OK) { jn_sgm_destroy(h); return e; }
  *out = h;
  return JN_OK;
}

jn_status jn_sgm_create(const jn_sgm_params* p, int32_t W, int32_t H, int32_t max_batch, int32_t device, jn_sgm** out) {
  const jn_sgm_cost_params sad3 = {JN_SGM_COST_SAD3, 0, 0, 0};
  return jn_sgm_create_cost(p, &sad3, W, H, max_batch, device, out);
}

jn_status jn_sgm_cost_volume(jn_sgm* h, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch, int64_t image_stride, uint8_t* dCost) {
  if (!h || n < 1 || n > h->max_batch || !dI1 || !dI2 || !dCost || ((uintptr_t)dCost & 15) || pitch < h->W) return JN_ERR_INVALID;
  if (!h->makes_volume()) return JN_ERR_UNSUPPORTED;
  return sgm_run_sync(h, false, [&](jn_sgm::Slot& s) { return sgm_queue_volume(h, s, n, dI1, dI2, pitch, (long long)image_stride, dCost); });
}

jn_status jn_sgm_aggregate_batch(jn_sgm* h, int32_t n, const uint8_t* dCost, int16_t* dDisp) {
  if (!h || n < 1 || n > h->max_batch || !dCost || ((uintptr_t)dCost & 15) || !dDisp) return JN_ERR_INVALID;
  if (h->cost.cost_function == JN_SGM_COST_SAD3) return JN_ERR_UNSUPPORTED;
  return sgm_run_sync(h, true, [&](jn_sgm::Slot& s) {
    const hipError_t e = hipEventRecord(s.ev[0], s.stream);
    return e != hipSuccess ? e : jnav_sgm::sweep_run_cost(h->sw, n, dCost, dDisp, s.stream, s.sb, s.ev, true);
  });
}

jn_status jn_sgm_process_batch(jn_sgm* h, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch, int64_t image_stride, int16_t* dDisp) {
  if (!h || n < 1 || n > h->max_batch || !dI1 || !dI2 || !dDisp || pitch < h->W) return JN_ERR_INVALID;
  if (h->cost.cost_function == JN_SGM_COST_EXTERNAL) return JN_ERR_UNSUPPORTED;   // the handle only aggregates (jn_sgm_aggregate_batch)
  return sgm_run_sync(h, true, [&](jn_sgm::Slot& s) { return sgm_queue(h, s, n, dI1, dI2, pitch, (long long)image_stride, dDisp, true, true); });
}

jn_status jn_sgm_submit_scan(jn_sgm* h, int32_t slot, int32_t n, const uint8_t* dI1, const uint8_t* dI2, int32_t pitch, int64_t image_stride, int16_t* dDisp,
                             const jn_scan_params* sp, const uint8_t* dLut, uint8_t* dDispU8, double* dBins, double* dMeta) {
  if (!h || slot < 0 || slot >= jn_sgm::kSgmSlots || n < 1 || n > h->max_batch || !dI1 || !dI2 || !dDisp || pitch < h->W) return JN_ERR_INVALID;
  if (sp && (!dLut || !dDispU8 || !dBins || !dMeta || sp->bins < 1 || sp->bins > 1024)) return JN_ERR_INVALID;
  if (h->cost.cost_function == JN_SGM_COST_EXTERNAL) return JN_ERR_UNSUPPORTED;
  jn_sgm::Slot& s = h->slots[slot];
  if (s.pending) return JN_ERR_INVALID;                         // one batch per slot: jn_sgm_wait first
  HIP_TRY(hipSetDevice(h->device));
  const jn_status es = sgm_make_slot(h, slot);
  if (es != JN_OK) return es;
  if (sp && !s.scan_scratch) HIP_TRY(s.own.alloc(&s.scan_scratch, (size_t)4 * h->max_batch));
  jnav_sgm::SweepBuffers& sb = s.sb;
  hipStream_t st = s.stream;
  // With a scan: ONE tail kernel applies the L/R check, writes the int16 map and the mono8 map (point_cloud.cpp:422 semantics) and scans
  // (JN_SGM_TAIL=3: the three kernels k_sw_lr, k_sgm_to_u8, k_scan one after the other, for A/B).
  static const bool fused_tail = !(getenv("JN_SGM_TAIL") && atoi(getenv("JN_SGM_TAIL")) == 3);
  // An attached post-filter (include/jn_postfilter.h) sits between the L/R check and everything that reads the map, so the one-kernel tail
  // cannot be used: such a slot queues the three kernels, with the filter in place on dDisp behind the first.
  const jnav::NavTails& tails = s.tails;
  const bool fuse = sp && fused_tail && !tails.pf.on;
  HIP_TRY(sgm_queue(h, s, n, dI1, dI2, pitch, (long long)image_stride, dDisp, false, !fuse));
  HIP_TRY(tails.launch_postfilter_in_place(st, n, dDisp, h->W, h->H));
  if (fuse) {
    jnav::SgmWinners w;
    w.dl = sb.dl; w.minr = sb.minr; w.disp = dDisp; w.lr = h->sw.lr; w.subpixel = h->sw.subpixel;
    jnav::launch_scan(st, *sp, n, nullptr, dDispU8, dLut, h->W, h->H, dBins, dMeta, s.scan_scratch, nullptr, &w);
  } else if (sp) {
    const long long px = (long long)n * h->W * h->H;
    hipLaunchKernelGGL(k_sgm_to_u8, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, dDisp, h->p.subpixel ? 1 : 0, dDispU8, px);
    jnav::launch_scan(st, *sp, n, nullptr, dDispU8, dLut, h->W, h->H, dBins, dMeta, s.scan_scratch);
  }
  if (sp) {                                                     // the attached tails: the costmap of the mono8 map and the bins just written, the sub-pixel tail of the int16 map
    const int native = h->p.subpixel ? JN_DISP_I16_SUB : JN_DISP_I16;
    HIP_TRY(tails.launch(st, *sp, n, dDispU8, dLut, dBins, dDisp, native, h->W, h->H));
  }
  // the batch's end: behind the scan tail, not behind the sweeps (ev[3] stays the end of the winner-takes-all timing)
  if (!s.ev_end) HIP_TRY(s.own.event(&s.ev_end, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(s.ev_end, st));
  HIP_TRY(hipGetLastError());
  s.pending = true;
  return JN_OK;
}

jn_status jn_sgm_attach_costmap(jn_sgm* h, int32_t slot, const jn_costmap_params* cp, uint16_t* dHits, int8_t* dGrid) {
  if (!h || slot < 0 || slot >= jn_sgm::kSgmSlots) return JN_ERR_INVALID;
  if (h->slots[slot].pending) return JN_ERR_INVALID;            // a batch is in flight on the slot: jn_sgm_wait first
  return h->slots[slot].tails.attach_costmap(h->device, h->max_batch, cp, dHits, dGrid);
}

jn_status jn_sgm_attach_subpix(jn_sgm* h, int32_t slot, const jn_costmap_params* cp, double* dBins, double* dMeta, uint16_t* dHits, int8_t* dGrid) {
  if (!h || slot < 0 || slot >= jn_sgm::kSgmSlots) return JN_ERR_INVALID;
  if (h->slots[slot].pending) return JN_ERR_INVALID;            // a batch is in flight on the slot: jn_sgm_wait first
  return h->slots[slot].tails.attach_subpix(h->device, h->max_batch, cp, dBins, dMeta, dHits, dGrid);
}

jn_status jn_sgm_attach_postfilter(jn_sgm* h, int32_t slot, const jn_postfilter_params* fp, uint32_t* dStats) {
  if (!h || slot < 0 || slot >= jn_sgm::kSgmSlots) return JN_ERR_INVALID;
  if (h->slots[slot].pending) return JN_ERR_INVALID;            // a batch is in flight on the slot: jn_sgm_wait first
  return h->slots[slot].tails.attach_postfilter(h->device, h->max_batch, h->W, h->H, h->p.subpixel ? JN_DISP_I16_SUB : JN_DISP_I16, fp, dStats);
}

jn_status jn_sgm_wait(jn_sgm* h, int32_t slot) {
  if (!h || slot < 0 || slot >= jn_sgm::kSgmSlots) return JN_ERR_INVALID;
  jn_sgm::Slot& s = h->slots[slot];
  if (!s.pending) return JN_OK;
  HIP_TRY(hipSetDevice(h->device));
  s.pending = false;
  HIP_TRY(hipEventSynchronize(s.ev_end));                       // the slot's own end, scan tail included (its stream may carry a later slot's batch)
  HIP_TRY(hipGetLastError());
  sgm_read_times(h, s);
  return JN_OK;
}

const void* jn_sgm_debug_ptr(jn_sgm* h, int32_t which, int32_t info[5]) {
  if (!h) return nullptr;
  if (info) { info[0] = h->sw.wide; info[1] = h->sw.Wp; info[2] = h->sw.padl; info[3] = h->sw.NB; info[4] = 1; }
  const jnav_sgm::SweepBuffers& sb = h->slots[0].sb;
  switch (which) {
    case 0: return sb.volF; case 1: return sb.volH0; case 2: return sb.volH1;
    case 3: return sb.minr; case 4: return sb.dl; case 5: return sb.gm;
  }
  return nullptr;
}

jn_status jn_sgm_last_times(jn_sgm* h, jn_sgm_times* out) {
  if (!h || !out) return JN_ERR_INVALID;
  *out = h->times;
  return JN_OK;
}

jn_status jn_sgm_disparity_to_u8(int32_t device, const int16_t* dDisp, int32_t subpixel, uint8_t* dOut, int64_t n) {
  if (!dDisp || !dOut || n < 0) return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  if (n) hipLaunchKernelGGL(k_sgm_to_u8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dDisp, subpixel ? 1 : 0, dOut, (long long)n);
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // extern "C"

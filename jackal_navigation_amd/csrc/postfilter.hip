// postfilter.hip — the disparity post-filter (include/jn_postfilter.h): speckle removal by connected components, then an optional 3x3
// median, on the int16 maps of the SGM and block-matching modes.  Product code.
//
// No reference counterpart; the definition is in jn_postfilter.h and its scalar restatement (the checker, tests/postfilter_def.py) lives
// in the tests.  Everything is integer arithmetic and no result depends on the order pixels are visited in, so the bar is bit-identity.
//
// Shape: separate launches on one stream; no workgroup ever waits for another one.
//   k_pf_label_tile     a 64 x 32 tile per workgroup, lanes = columns.  Rows become runs by ballots, runs are united vertically in LDS,
//                       and every pixel gets the frame index of its tile segment's smallest pixel (label[p]; a tile root has
//                       label[p] == p).  size[p] = pixels of the tile segment at its root, 0 everywhere else.
//   k_pf_merge_borders  one thread per pixel next to a tile border: unites the tile roots of connected neighbours in global memory.
//   k_pf_resolve        every tile root (size[p] != 0) finds its segment's root, points at it, and adds its pixels to the root's size:
//                       one atomicAdd per tile root, not per pixel.
//   k_pf_apply          label -> tile root -> root -> size, the threshold, the output, the statistics; 8 pixels per 16-byte access.
//   k_pf_apply_median   the same decision for a 128 x 16 tile and its one-pixel border into LDS, the median from there: stage 1's
//                       output never goes to memory.
// Union-find: a label array in which label[p] <= p always holds and a root has label[p] == p.  find() follows labels, which strictly
// decrease until a root; unite() replaces the larger root's label by atomicMin and, when it lost a race (the value it replaced was not
// the root itself), goes on with the label it displaced — the pair (a, b) strictly decreases with every round, so every loop here
// terminates whatever the other threads do, and nothing is ever locked.  A stale read only returns an older ancestor of the same set.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/jn_postfilter.h"
#include "nav_tail.h"

namespace jnav {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;          // label of an invalid pixel
constexpr int kTW = 64, kTH = 32;                // label tile: one wave per row segment, 8 rows per wave
constexpr int kRowsPerWave = kTH / 4;
constexpr int kMW = 128, kMH = 16;               // median tile: 8 pixels per thread
constexpr int kMaxFramesPerLaunch = 32768;       // gridDim.y / .z

struct PfStats { uint32_t valid, segments, speckles, removed; };

DEV bool pf_conn(int a, int b, int thr) { return a >= 0 && b >= 0 && abs(a - b) <= thr; }

// labels strictly decrease along the chain: terminates
DEV uint32_t pf_find_lds(const uint32_t* lab, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
DEV uint32_t pf_find(const uint32_t* lab, uint32_t x) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
// a + b strictly decreases with every round that does not return (see the head of the file)
DEV void pf_unite_lds(uint32_t* lab, uint32_t a, uint32_t b) {
  for (;;) {
    a = pf_find_lds(lab, a); b = pf_find_lds(lab, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}
DEV void pf_unite(uint32_t* lab, uint32_t a, uint32_t b) {
  for (;;) {
    a = pf_find(lab, a); b = pf_find(lab, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

// Adds the workgroup's statistics to the frame's: wave sums by shuffles, one LDS add per wave, one global add per workgroup and field.
DEV void pf_add_stats(PfStats s, uint32_t* lds4, uint32_t* __restrict__ gstats) {
  if (threadIdx.x < 4) lds4[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    s.valid += __shfl_xor(s.valid, off); s.segments += __shfl_xor(s.segments, off);
    s.speckles += __shfl_xor(s.speckles, off); s.removed += __shfl_xor(s.removed, off);
  }
  if ((threadIdx.x & 63) == 0) {
    if (s.valid) atomicAdd(&lds4[0], s.valid);
    if (s.segments) atomicAdd(&lds4[1], s.segments);
    if (s.speckles) atomicAdd(&lds4[2], s.speckles);
    if (s.removed) atomicAdd(&lds4[3], s.removed);
  }
  __syncthreads();
  if (threadIdx.x < 4 && lds4[threadIdx.x]) atomicAdd(&gstats[threadIdx.x], lds4[threadIdx.x]);
}

// grid (tiles_x, tiles_y, n).  Lane = column of the tile, wave w = rows 8 w .. 8 w + 7.
__global__ void __launch_bounds__(256) k_pf_label_tile(const int16_t* __restrict__ in, int W, int H, int thr, uint32_t* __restrict__ label,
                                                       uint32_t* __restrict__ size) {
  __shared__ uint32_t lab[kTW * kTH];
  __shared__ uint32_t siz[kTW * kTH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH;
  const int x = tx0 + lane, r0 = wave * kRowsPerWave;
  const size_t fb = (size_t)blockIdx.z * W * H;
  const int16_t* __restrict__ f = in + fb;
  const bool inx = x < W;
  // the row above the wave's first one, when it is a row of this tile
  int vu = -1;
  if (inx && wave > 0 && ty0 + r0 - 1 < H) vu = f[(size_t)(ty0 + r0 - 1) * W + x];
  unsigned long long hu;
  {
    const int left = __shfl_up(vu, 1);
    hu = __ballot(lane > 0 && pf_conn(vu, left, thr));
  }
  uint32_t need = 0;                                            // bit i: row r0 + i has to be united with the pixel above
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    const int r = r0 + i, y = ty0 + r;
    const int v = (inx && y < H) ? (int)f[(size_t)y * W + x] : -1;
    const int left = __shfl_up(v, 1);
    const bool ch = lane > 0 && pf_conn(v, left, thr);          // connected to the left neighbour
    const unsigned long long h = __ballot(ch);
    // the run's first column: the highest lane at or below this one that is not connected to its left
    const unsigned long long starts = ~h & ((2ull << lane) - 1ull);
    const int start = 63 - __clzll((long long)starts);
    const int li = r * kTW + lane;
    lab[li] = v >= 0 ? (uint32_t)(r * kTW + start) : kNone;
    siz[li] = 0;
    const bool cu = r > 0 && pf_conn(v, vu, thr);               // connected to the pixel above (same tile)
    const unsigned long long vm = __ballot(cu);
    // implied by the left neighbour's union when both runs continue: left ~ this, up-left ~ up, left ~ up-left
    const bool implied = ch && ((vm >> (lane - 1)) & 1ull) && ((hu >> lane) & 1ull);
    if (cu && !implied) need |= 1u << i;
    vu = v; hu = h;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++)
    if ((need >> i) & 1u) { const int li = (r0 + i) * kTW + lane; pf_unite_lds(lab, (uint32_t)li, (uint32_t)(li - kTW)); }
  __syncthreads();
  uint32_t root[kRowsPerWave];
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    const int li = (r0 + i) * kTW + lane;
    const uint32_t l = lab[li];
    const uint32_t rt = l == kNone ? kNone : pf_find_lds(lab, l);
    root[i] = rt;
    // one LDS add per stretch of neighbouring lanes with the same root
    const uint32_t prev = __shfl_up(rt, 1);
    const unsigned long long first = __ballot(lane == 0 || rt != prev);
    if (rt != kNone && ((first >> lane) & 1ull)) {
      const unsigned long long rest = lane == 63 ? 0ull : first >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;
      atomicAdd(&siz[rt], (uint32_t)len);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    const int r = r0 + i, y = ty0 + r;
    if (!inx || y >= H) continue;
    const size_t g = fb + (size_t)y * W + x;
    const uint32_t rt = root[i];
    label[g] = rt == kNone ? kNone : (uint32_t)((ty0 + (int)(rt / kTW)) * W + tx0 + (int)(rt % kTW));
    size[g] = siz[r * kTW + lane];
  }
}

// grid (ceil(items / 256), 1, n); items = the pixels below a horizontal tile border, then the pixels right of a vertical one.
__global__ void __launch_bounds__(256) k_pf_merge_borders(const int16_t* __restrict__ in, int W, int H, int thr, int nhb, int items,
                                                          uint32_t* __restrict__ label) {
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= items) return;
  const size_t fb = (size_t)blockIdx.z * W * H;
  const int16_t* __restrict__ f = in + fb;
  uint32_t* lab = label + fb;
  int x, y, ox, oy;                                            // the pixel, and its neighbour across the border
  bool inner;                                                  // the pixel before it along the border lies in the same pair of tiles
  if (idx < nhb * W) { y = (idx / W + 1) * kTH; x = idx % W; ox = x; oy = y - 1; inner = x % kTW != 0; }
  else { idx -= nhb * W; x = (idx / H + 1) * kTW; y = idx % H; ox = x - 1; oy = y; inner = y % kTH != 0; }
  const int v = f[(size_t)y * W + x], o = f[(size_t)oy * W + ox];
  if (!pf_conn(v, o, thr)) return;
  if (inner) {                                                 // implied by the union of the pair before this one (as in k_pf_label_tile)
    const int px = x - (oy == y ? 0 : 1), py = y - (oy == y ? 1 : 0), pox = ox - (oy == y ? 0 : 1), poy = oy - (oy == y ? 1 : 0);
    const int pv = f[(size_t)py * W + px], po = f[(size_t)poy * W + pox];
    if (pf_conn(v, pv, thr) && pf_conn(o, po, thr) && pf_conn(pv, po, thr)) return;
  }
  pf_unite(lab, lab[(size_t)y * W + x], lab[(size_t)oy * W + ox]);
}

// grid (ceil(W H / 256), n).  After it every tile root points at its segment's root, whose size is the segment's.
__global__ void __launch_bounds__(256) k_pf_resolve(int WH, uint32_t* __restrict__ label, uint32_t* __restrict__ size) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)WH) return;
  const size_t fb = (size_t)blockIdx.y * WH;
  const uint32_t c = size[fb + p];
  if (c == 0) return;                                           // not a tile root
  const uint32_t r = pf_find(label + fb, p);
  if (r == p) return;
  label[fb + p] = r;                                            // r is the root for good: the unions are complete
  atomicAdd(&size[fb + r], c);
}

// What stage 1 makes of pixel p (frame index) with value v >= 0: the value, or the marker.  Counts a root once, at its own pixel.
DEV int pf_decide(const uint32_t* __restrict__ lab, const uint32_t* __restrict__ siz, uint32_t p, int v, int speckle_size, int marker,
                  bool count, PfStats& st) {
  const uint32_t t = lab[p];
  const uint32_t r = t == p ? p : lab[t];                       // pixel -> tile root -> root (k_pf_resolve)
  const uint32_t c = siz[r];
  const bool speckle = c < (uint32_t)speckle_size;
  if (count && r == p) { st.segments++; if (speckle) { st.speckles++; st.removed += c; } }
  return speckle ? marker : v;
}

// grid (ceil(groups / 256), n): a thread takes one 16-byte group of 8 pixels of the whole batch; the groups a frame shares with its
// neighbours (W H not a multiple of 8) are taken pixel by pixel by each of the two frames.
template <bool kVec>
__global__ void __launch_bounds__(256) k_pf_apply(const int16_t* in, int WH, int speckle_size, int marker, const uint32_t* __restrict__ label,
                                                  const uint32_t* __restrict__ size, int16_t* out, uint32_t* __restrict__ stats) {
  __shared__ uint32_t red[4];
  const size_t fb = (size_t)blockIdx.y * WH;
  const size_t g = (fb >> 3) + (size_t)blockIdx.x * 256 + threadIdx.x;     // group of the batch
  const size_t lo = std::max(g * 8, fb), hi = std::min(g * 8 + 8, fb + (size_t)WH);
  const uint32_t* __restrict__ lab = label + fb;
  const uint32_t* __restrict__ siz = size + fb;
  PfStats st = {0, 0, 0, 0};
  if (lo < hi) {
    if (kVec && hi - lo == 8) {
      const int4 raw = *reinterpret_cast<const int4*>(in + lo);
      int16_t v[8];
      __builtin_memcpy(v, &raw, 16);
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (v[k] >= 0) { st.valid++; if (speckle_size > 0) v[k] = (int16_t)pf_decide(lab, siz, (uint32_t)(lo - fb) + k, v[k], speckle_size, marker, true, st); }
      int4 res;
      __builtin_memcpy(&res, v, 16);
      *reinterpret_cast<int4*>(out + lo) = res;
    } else {
      for (size_t e = lo; e < hi; e++) {
        int v = in[e];
        if (v >= 0) { st.valid++; if (speckle_size > 0) v = pf_decide(lab, siz, (uint32_t)(e - fb), v, speckle_size, marker, true, st); }
        out[e] = (int16_t)v;
      }
    }
  }
  if (stats) pf_add_stats(st, red, stats + 4 * (size_t)blockIdx.y);
}

DEV void pf_cswap(int& a, int& b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }

// grid (tiles_x * tiles_y, n).  Stage 1's output of the tile and its border goes to LDS (invalid on input: the value itself, < 0; removed:
// the marker; outside the image: -1); a thread then takes 8 neighbouring pixels of one row.
template <bool kSpeckle, bool kVec>
__global__ void __launch_bounds__(256) k_pf_apply_median(const int16_t* __restrict__ in, int W, int H, int tiles_x, int speckle_size, int marker,
                                                         const uint32_t* __restrict__ label, const uint32_t* __restrict__ size,
                                                         int16_t* __restrict__ out, uint32_t* __restrict__ stats) {
  constexpr int LW = kMW + 2, LH = kMH + 2;
  __shared__ int16_t tile[LH * LW];
  __shared__ uint32_t red[4];
  const int tx0 = (blockIdx.x % tiles_x) * kMW, ty0 = (blockIdx.x / tiles_x) * kMH;
  const size_t fb = (size_t)blockIdx.y * W * H;
  const int16_t* __restrict__ f = in + fb;
  const uint32_t* __restrict__ lab = label + fb;
  const uint32_t* __restrict__ siz = size + fb;
  PfStats st = {0, 0, 0, 0};
  for (int e = threadIdx.x; e < LH * LW; e += 256) {
    const int ly = e / LW, lx = e % LW;
    const int x = tx0 + lx - 1, y = ty0 + ly - 1;
    int v = -1;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      const bool own = lx >= 1 && lx <= kMW && ly >= 1 && ly <= kMH;
      v = f[(size_t)y * W + x];
      if (v >= 0) {
        if (own) st.valid++;
        if (kSpeckle) v = pf_decide(lab, siz, (uint32_t)(y * W + x), v, speckle_size, marker, own, st);
      }
    }
    tile[e] = (int16_t)v;
  }
  __syncthreads();
  const int ly = threadIdx.x / (kMW / 8), lx0 = (threadIdx.x % (kMW / 8)) * 8;
  const int y = ty0 + ly, x0 = tx0 + lx0;
  if (y < H && x0 < W) {
    int16_t res[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int16_t* c = &tile[(ly + 1) * LW + lx0 + k + 1];
      const int cv = c[0];
      int s[9];
      int cnt = 0;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          const int w = c[dy * LW + dx];
          s[(dy + 1) * 3 + dx + 1] = w >= 0 ? w : 0x7FFFFFFF;     // invalid values sort behind every valid one
          cnt += w >= 0 ? 1 : 0;
        }
      // odd-even transposition: nine rounds sort nine values
#pragma unroll
      for (int round = 0; round < 9; round++)
#pragma unroll
        for (int i = round & 1; i + 1 < 9; i += 2) pf_cswap(s[i], s[i + 1]);
      const int m = (cnt - 1) >> 1;                             // 0 .. 4 for a valid centre
      const int med = m == 0 ? s[0] : m == 1 ? s[1] : m == 2 ? s[2] : m == 3 ? s[3] : s[4];
      res[k] = (int16_t)(cv >= 0 ? med : cv);
    }
    int16_t* o = out + fb + (size_t)y * W + x0;
    if (kVec && x0 + 8 <= W) {
      int4 r4;
      __builtin_memcpy(&r4, res, 16);
      *reinterpret_cast<int4*>(o) = r4;
    } else {
      for (int k = 0; k < 8 && x0 + k < W; k++) o[k] = res[k];
    }
  }
  if (stats) pf_add_stats(st, red, stats + 4 * (size_t)blockIdx.y);
}

inline size_t pf_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

bool postfilter_params_valid(const jn_postfilter_params* fp) {
  return fp && (fp->format == JN_DISP_I16 || fp->format == JN_DISP_I16_SUB) && fp->speckle_size >= 0 &&
         fp->speckle_size <= JN_POSTFILTER_MAX_SPECKLE_SIZE && fp->speckle_range_q >= 0 && fp->speckle_range_q <= JN_POSTFILTER_MAX_RANGE_Q &&
         (fp->median == 0 || fp->median == 1);
}

size_t postfilter_scratch_bytes(const jn_postfilter_params& fp, int n, int W, int H, bool in_place) {
  const size_t px = (size_t)std::min(n, kMaxFramesPerLaunch) * W * H;
  size_t b = 256;
  if (fp.speckle_size > 0) b += 2 * pf_align(px * sizeof(uint32_t));
  if (fp.median && in_place) b += pf_align(px * sizeof(int16_t));
  return b;
}

hipError_t launch_postfilter(hipStream_t st, const jn_postfilter_params& fp, int n, const int16_t* in, int W, int H, int16_t* out, uint32_t* stats,
                             void* scratch) {
  const size_t WH = (size_t)W * H;
  const bool speckle = fp.speckle_size > 0, median = fp.median != 0, in_place = in == out;
  const int thr = fp.format == JN_DISP_I16 ? fp.speckle_range_q / 16 : fp.speckle_range_q;    // |16 a - 16 b| <= r  <=>  |a - b| <= r / 16
  const int marker = fp.format == JN_DISP_I16 ? -1 : -16;
  if (stats) {
    const hipError_t e = hipMemsetAsync(stats, 0, sizeof(uint32_t) * 4 * (size_t)n, st);      // on the SAME stream as the kernels that add to it
    if (e != hipSuccess) return e;
  }
  for (int n0 = 0; n0 < n; n0 += kMaxFramesPerLaunch) {         // the frames are independent: batches beyond the grid's reach go in parts
    const int m = std::min(n - n0, kMaxFramesPerLaunch);
    const size_t px = (size_t)m * WH;
    const int16_t* cin = in + (size_t)n0 * WH;
    int16_t* cout = out + (size_t)n0 * WH;
    uint32_t* cstats = stats ? stats + 4 * (size_t)n0 : nullptr;
    char* s = static_cast<char*>(scratch);
    uint32_t* label = nullptr;
    uint32_t* size = nullptr;
    if (speckle) { label = reinterpret_cast<uint32_t*>(s); s += pf_align(px * 4); size = reinterpret_cast<uint32_t*>(s); s += pf_align(px * 4); }
    int16_t* dst = (median && in_place) ? reinterpret_cast<int16_t*>(s) : cout;
    const bool vec = ((reinterpret_cast<uintptr_t>(cin) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (speckle) {
      hipLaunchKernelGGL(k_pf_label_tile, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, m), dim3(256), 0, st, cin, W, H, thr, label, size);
      const int nhb = (H - 1) / kTH, nvb = (W - 1) / kTW, items = nhb * W + nvb * H;
      if (items > 0) hipLaunchKernelGGL(k_pf_merge_borders, dim3((items + 255) / 256, 1, m), dim3(256), 0, st, cin, W, H, thr, nhb, items, label);
      hipLaunchKernelGGL(k_pf_resolve, dim3((unsigned)((WH + 255) / 256), m), dim3(256), 0, st, (int)WH, label, size);
    }
    if (median) {
      const int tiles_x = (W + kMW - 1) / kMW, tiles_y = (H + kMH - 1) / kMH;
      const dim3 g(tiles_x * tiles_y, m);
      const bool mvec = vec && W % 8 == 0;
      if (speckle) {
        if (mvec) hipLaunchKernelGGL((k_pf_apply_median<true, true>), g, dim3(256), 0, st, cin, W, H, tiles_x, fp.speckle_size, marker, label, size, dst, cstats);
        else hipLaunchKernelGGL((k_pf_apply_median<true, false>), g, dim3(256), 0, st, cin, W, H, tiles_x, fp.speckle_size, marker, label, size, dst, cstats);
      } else {
        if (mvec) hipLaunchKernelGGL((k_pf_apply_median<false, true>), g, dim3(256), 0, st, cin, W, H, tiles_x, 0, marker, label, size, dst, cstats);
        else hipLaunchKernelGGL((k_pf_apply_median<false, false>), g, dim3(256), 0, st, cin, W, H, tiles_x, 0, marker, label, size, dst, cstats);
      }
      if (dst != cout) {
        const hipError_t e = hipMemcpyAsync(cout, dst, px * sizeof(int16_t), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
      }
    } else if (speckle) {
      const unsigned groups = (unsigned)((WH + 7) / 8 + 1);
      const dim3 g((groups + 255) / 256, m);
      if (vec) hipLaunchKernelGGL((k_pf_apply<true>), g, dim3(256), 0, st, cin, (int)WH, fp.speckle_size, marker, label, size, cout, cstats);
      else hipLaunchKernelGGL((k_pf_apply<false>), g, dim3(256), 0, st, cin, (int)WH, fp.speckle_size, marker, label, size, cout, cstats);
    } else if (!in_place || cstats) {                           // nothing to do but the copy and the count of valid pixels (speckle_size 0: no labels are read)
      const unsigned groups = (unsigned)((WH + 7) / 8 + 1);
      const dim3 g((groups + 255) / 256, m);
      if (vec) hipLaunchKernelGGL((k_pf_apply<true>), g, dim3(256), 0, st, cin, (int)WH, 0, marker, label, size, cout, cstats);
      else hipLaunchKernelGGL((k_pf_apply<false>), g, dim3(256), 0, st, cin, (int)WH, 0, marker, label, size, cout, cstats);
    }
  }
  return hipSuccess;
}

}  // namespace jnav

using namespace jnav;

extern "C" {

void jn_postfilter_params_default(jn_postfilter_params* fp, int32_t format) {
  fp->format = format; fp->speckle_size = 200; fp->speckle_range_q = 16; fp->median = 0;
}

jn_status jn_disparity_postfilter(int32_t device, const jn_postfilter_params* fp, int32_t n, const int16_t* dIn, int32_t W, int32_t H,
                                  int16_t* dOut, uint32_t* dStats) {
  if (!postfilter_params_valid(fp) || !dIn || !dOut || n < 1 || W < 1 || H < 1 || W > JN_POSTFILTER_MAX_SIDE || H > JN_POSTFILTER_MAX_SIDE)
    return JN_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  void* scratch = nullptr;
  HIP_TRY(thread_scratch(device, postfilter_scratch_bytes(*fp, n, W, H, dIn == dOut), &scratch));
  HIP_TRY(launch_postfilter(nullptr, *fp, n, dIn, W, H, dOut, dStats, scratch));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipGetLastError());
  return JN_OK;
}

}  // extern "C"

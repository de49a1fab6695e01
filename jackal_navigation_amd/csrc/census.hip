// census.hip — the census / Hamming cost volume of the SGM mode (include/jn_sgm_cost.h, JN_SGM_COST_CENSUS).  Product code.
//
// Two kernels.  k_census<RX, RY> turns the raw u8 images of both eyes into one 64-bit signature per pixel (bit set = that neighbour of
// the (2 RX + 1) x (2 RY + 1) window is strictly darker than the centre; replicated borders).  k_census_volume<D, CLAMP> writes
// C(x, y, d) = min(popcount(cen_L(x, y) ^ cen_R(max(x - d, 0), y)), cost_max) as bytes [n][H][W][D].  Only Hamming distances leave this
// file: the order of a signature's bits is whatever the unrolled loops below make it.
//
// The volume kernel is the hot one (it writes n H W D bytes).  A lane owns (pixel, chunk of 16 disparities): its 16 cost bytes are one
// 16-byte store, the lanes of a wave write 1 KB contiguous, and no transposition is needed.  The right signatures of a tile of 256
// columns (and the D columns to its left) are staged once in LDS; a lane reads its 16, one 8-byte slot apart, with ds_read_b64.  In the
// natural lane order the 32 lanes of a half-wave are 512 / D pixels x D / 16 chunks, and their columns p - 16 c - t fall on only 512 / D
// distinct slots modulo 32.  Leaving PAD = 512 / D empty slots after every 16 columns (slot = j + PAD (j >> 4)) makes a chunk step
// 16 + PAD = PAD x odd slots, which spreads the chunks over the multiples of PAD, and a 16-column boundary inside the pixels of a
// half-wave shifts by PAD, which keeps them distinct modulo PAD: the 32 slots are distinct modulo 32 for every D.  The padding moves
// the conflicts to the staging writes (32 consecutive columns collide 32 / PAD-way on ds_write_b64): one or two writes per lane and
// tile against 16 reads per lane and pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "census.h"

namespace jnav_census {

namespace {

constexpr int kTileW = 128, kTileH = 8;            // k_census: pixels of a workgroup (4 consecutive columns per lane)
constexpr int kHalo = 4;                           // staged columns left and right of the tile: >= RX, a whole dword

// ---- the census transform: img < n left images, the others right ones ----
template <int RX, int RY>
__global__ void __launch_bounds__(256) k_census(CDev s, int n, const uint8_t* __restrict__ I1, const uint8_t* __restrict__ I2, int pitch, long long stride,
                                                uint64_t* __restrict__ sig) {
  constexpr int ROWS = kTileH + 2 * RY, LW = (kTileW + 2 * kHalo) / 4;     // staged rows, dwords per staged row
  __shared__ uint32_t tile[ROWS][LW];
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, img = blockIdx.z;
  const uint8_t* I = img < n ? I1 + (long long)img * stride : I2 + (long long)(img - n) * stride;
  // A dword load where the caller's base and pitch are dword aligned (uniform over the launch) and the dword lies inside the row;
  // elsewhere, and at the left and right borders, bytes clamped one by one.
  const bool aligned = ((reinterpret_cast<uintptr_t>(I) | (uintptr_t)pitch) & 3) == 0;
  for (int i = threadIdx.x; i < ROWS * LW; i += 256) {
    const int r = i / LW, q = i - r * LW;
    const uint8_t* row = I + (size_t)min(max(y0 + r - RY, 0), s.H - 1) * pitch;
    const int xb = x0 - kHalo + 4 * q;                                     // a multiple of 4
    uint32_t w = 0;
    if (aligned && xb >= 0 && xb + 3 < s.W) w = *reinterpret_cast<const uint32_t*>(row + xb);
    else {
#pragma unroll
      for (int k = 0; k < 4; k++) w |= (uint32_t)row[min(max(xb + k, 0), s.W - 1)] << (8 * k);
    }
    tile[r][q] = w;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 5, tq = threadIdx.x & 31;
  const int y = y0 + ty, x = x0 + 4 * tq;
  if (y >= s.H || x >= s.W) return;
  uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
  const uint32_t cw = tile[ty + RY][tq + 1];                               // the four centres
#pragma unroll
  for (int j = 0; j <= 2 * RY; j++) {
    const uint32_t d[3] = {tile[ty + j][tq], tile[ty + j][tq + 1], tile[ty + j][tq + 2]};   // columns x - 4 .. x + 7
#pragma unroll
    for (int i = -RX; i <= RX; i++) {
      if (j == RY && i == 0) continue;
      constexpr int kFirstHalf = ((2 * RX + 1) * (2 * RY + 1) - 1) / 2;
      const int bit = j * (2 * RX + 1) + i + RX - ((j > RY || (j == RY && i > 0)) ? 1 : 0);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int b = kHalo + k + i;                                       // byte of the 12
        const uint32_t v = (d[b >> 2] >> (8 * (b & 3))) & 0xFFu, c = (cw >> (8 * k)) & 0xFFu;
        if (bit < kFirstHalf) lo[k] = lo[k] + lo[k] + (v < c ? 1u : 0u);
        else hi[k] = hi[k] + hi[k] + (v < c ? 1u : 0u);
      }
    }
  }
  uint64_t* out = sig + ((size_t)img * s.H + y) * s.W + x;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (x + k < s.W) out[k] = ((uint64_t)hi[k] << 32) | lo[k];
}

// ---- the volume ----
constexpr int kVolT = 256;                         // columns of a workgroup's tile (one row)

template <int D>
__device__ __forceinline__ int vol_slot(int j) { return j + (512 / D) * (j >> 4); }

template <int D, bool CLAMP>
__global__ void __launch_bounds__(256) k_census_volume(CDev s, int n, const uint64_t* __restrict__ sig, int cost_max, uint8_t* __restrict__ cost) {
  constexpr int CH = D / 16, PPP = 256 / CH, PASSES = kVolT / PPP;         // chunks per pixel, pixels per pass, passes
  constexpr int NS = kVolT + D, PAD = 512 / D;                             // staged right columns x0 - D .. x0 + T - 1
  constexpr int SLOTS = NS + PAD * (NS / 16);
  constexpr int PASS_SLOTS = PPP + PAD * (PPP / 16);                       // PPP is a multiple of 16: a pass moves every read by this many slots
  __shared__ uint64_t sr[SLOTS];
  const int x0 = blockIdx.x * kVolT, y = blockIdx.y, b = blockIdx.z;
  const uint64_t* sl = sig + ((size_t)b * s.H + y) * s.W;
  const uint64_t* sg = sig + ((size_t)(n + b) * s.H + y) * s.W;
  for (int j = threadIdx.x; j < NS; j += 256) sr[vol_slot<D>(j)] = sg[min(max(x0 - D + j, 0), s.W - 1)];
  __syncthreads();
  const int p = threadIdx.x / CH, c = threadIdx.x % CH;
  // the lane's 16 slots of pass 0 (column x0 + p - 16 c - t at staged index p + D - 16 c - t); a later pass adds a constant
  int rd[16];
#pragma unroll
  for (int t = 0; t < 16; t++) rd[t] = vol_slot<D>(p + D - 16 * c - t);
  uint8_t* crow = cost + (((size_t)b * s.H + y) * s.W) * D + 16 * c;
#pragma unroll
  for (int pass = 0; pass < PASSES; pass++) {
    const int x = x0 + pass * PPP + p;
    if (x >= s.W) break;
    const uint64_t l = sl[x];
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t v = 0;
#pragma unroll
      for (int t = 3; t >= 0; t--) {
        uint32_t h = (uint32_t)__builtin_popcountll(l ^ sr[rd[4 * k + t] + pass * PASS_SLOTS]);
        if (CLAMP) h = min(h, (uint32_t)cost_max);
        v = (v << 8) | h;
      }
      w[k] = v;
    }
    *reinterpret_cast<uint4*>(crow + (size_t)x * D) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <int RX, int RY>
void launch_census(hipStream_t st, const CDev& s, int n, const uint8_t* dI1, const uint8_t* dI2, int pitch, long long stride, uint64_t* sig) {
  const dim3 grid((s.W + kTileW - 1) / kTileW, (s.H + kTileH - 1) / kTileH, 2 * n);
  hipLaunchKernelGGL((k_census<RX, RY>), grid, dim3(256), 0, st, s, n, dI1, dI2, pitch, stride, sig);
}

template <int D>
void launch_volume(hipStream_t st, const CDev& s, int n, const uint64_t* sig, int cost_max, uint8_t* cost) {
  const dim3 grid((s.W + kVolT - 1) / kVolT, s.H, n);
  // the clamp is a compile-time switch: off when it cannot bite
  if (cost_max < s.bits) hipLaunchKernelGGL((k_census_volume<D, true>), grid, dim3(256), 0, st, s, n, sig, cost_max, cost);
  else hipLaunchKernelGGL((k_census_volume<D, false>), grid, dim3(256), 0, st, s, n, sig, cost_max, cost);
}

}  // namespace

void geometry(int W, int H, int D, int block_radius, CDev* s, Sizes* z, int max_batch) {
  s->W = W; s->H = H; s->D = D;
  s->rx = block_radius; s->ry = block_radius < 3 ? block_radius : 3;
  s->bits = (2 * s->rx + 1) * (2 * s->ry + 1) - 1;
  z->sig = (size_t)2 * max_batch * H * W * sizeof(uint64_t);
}

hipError_t cost_volume(const CDev& s, int n, const uint8_t* dI1, const uint8_t* dI2, int pitch, long long stride, void* sig, int cost_max, uint8_t* cost,
                       hipStream_t st) {
  uint64_t* g = static_cast<uint64_t*>(sig);
  if (s.D != 64 && s.D != 128 && s.D != 256) return hipErrorInvalidValue;   // ahead of the first launch
  switch (s.rx) {
    case 2: launch_census<2, 2>(st, s, n, dI1, dI2, pitch, stride, g); break;
    case 3: launch_census<3, 3>(st, s, n, dI1, dI2, pitch, stride, g); break;
    case 4: launch_census<4, 3>(st, s, n, dI1, dI2, pitch, stride, g); break;
    default: return hipErrorInvalidValue;
  }
  switch (s.D) {
    case 64: launch_volume<64>(st, s, n, g, cost_max, cost); break;
    case 128: launch_volume<128>(st, s, n, g, cost_max, cost); break;
    case 256: launch_volume<256>(st, s, n, g, cost_max, cost); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace jnav_census

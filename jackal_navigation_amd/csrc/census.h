// census.h — host interface of the census / Hamming cost volume (census.hip: include/jn_sgm_cost.h's JN_SGM_COST_CENSUS) used by sgm.hip's C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace jnav_census {

struct CDev {
  int W, H, D;
  int rx, ry;        // the window: (2 rx + 1) x (2 ry + 1), rx = block_radius, ry = min(block_radius, 3)
  int bits;          // (2 rx + 1)(2 ry + 1) - 1: the largest Hamming distance
};
struct Sizes { size_t sig; };      // bytes: signatures [2 n][H][W] uint64 (left images first)

void geometry(int W, int H, int D, int block_radius, CDev* s, Sizes* z, int max_batch);

// Queues the census transform of both eyes (raw u8 images, caller's pitch / stride) and the volume min(Hamming, cost_max) of every pair
// 0 <= d < D against the right signature at column max(x - d, 0), as bytes of cost [n][H][W][D] (16-byte aligned), on `st`.
// s.D is 64, 128 or 256; sig is geometry()'s buffer.
hipError_t cost_volume(const CDev& s, int n, const uint8_t* dI1, const uint8_t* dI2, int pitch, long long stride, void* sig, int cost_max, uint8_t* cost,
                       hipStream_t st);

}  // namespace jnav_census

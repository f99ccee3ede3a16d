// What the kernels that walk a score vector with a u32 column beside it share (by_label.h, collapse.h): a thread's
// loads of one strip, and the wave's fold of the lanes that stand on one group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"

namespace svs {

// A thread's part of strip `strip` of THREADS * VPT * 4 rows: VPT groups of four consecutive rows, THREADS groups apart.
// Per group a 16-byte load of the four scores, one of their four column values (null column: every value is 0) and one
// nibble of the dead-row bitmap (null: no row is masked), every load requested before the first is used; a group past
// the end reads as zeros and is not live.  Both vectors are padded to a multiple of four rows.
template <int THREADS, int VPT>
struct ScoredStrip {
  float4 sc4[VPT];
  uint4 val4[VPT];
  uint32_t dead[VPT];
  int64_t base, n;
  __device__ __forceinline__ ScoredStrip(const float* scores, const uint32_t* values, const uint32_t* dead_bits, int64_t n_, int64_t strip)
      : base(strip * (THREADS * VPT) + threadIdx.x), n(n_) {
    const float4* s4 = (const float4*)scores;
    const uint4* v4 = (const uint4*)values;
    const int64_t n4 = (n + 3) >> 2;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int64_t i4 = group(j);
      const bool in = i4 < n4;
      sc4[j] = in ? s4[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
      val4[j] = (v4 && in) ? v4[i4] : make_uint4(0u, 0u, 0u, 0u);
      dead[j] = dead_nibble(in ? dead_bits : nullptr, i4);
    }
  }
  static __device__ __forceinline__ int64_t strips(int64_t n) { return (n + THREADS * VPT * 4 - 1) / (THREADS * VPT * 4); }
  __device__ __forceinline__ int64_t group(int j) const { return base + (int64_t)j * THREADS; }   // the float4 index of group j
  __device__ __forceinline__ int64_t row(int j, int e) const { return group(j) * 4 + e; }
  __device__ __forceinline__ float score(int j, int e) const { return e == 0 ? sc4[j].x : e == 1 ? sc4[j].y : e == 2 ? sc4[j].z : sc4[j].w; }
  __device__ __forceinline__ uint32_t value(int j, int e) const { return e == 0 ? val4[j].x : e == 1 ? val4[j].y : e == 2 ? val4[j].z : val4[j].w; }
  __device__ __forceinline__ bool live(int j, int e) const { return row(j, e) < n && !((dead[j] >> e) & 1u); }
};

// Every lane of the wave calls this (converged): peer = the lane stands on the wave's leading group, key32 = its score
// key (a real key is never 0).  Returns the ballot of the peers; *top = the lane is the one peer that speaks for them:
// the HIGHEST lane holding their largest key32 -- rows ascend with the lane, so it holds their largest 64-bit key.
__device__ __forceinline__ unsigned long long wave_fold_top(bool peer, uint32_t key32, bool* top) {
  const unsigned long long peers = __ballot(peer);
  *top = peer;
  if (peers & (peers - 1)) {   // two lanes or more (wave-uniform)
    uint32_t mx = peer ? key32 : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t t = (uint32_t)__shfl_xor((int)mx, off, 64);
      mx = t > mx ? t : mx;
    }
    const unsigned long long tops = __ballot(peer && key32 == mx);
    *top = (int)(threadIdx.x & 63) == 63 - __clzll((long long)tops);
  }
  return peers;
}

}  // namespace svs

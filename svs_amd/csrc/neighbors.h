// svs_index_neighbors: what runs in front of and behind an ordinary search when the queries are STORED ROWS.
//
//   rows_as_queries_kernel  a list of local rows -> the f32 query panel (nq x d, C-contiguous) the search then stages,
//                           converts and quantises like any host batch.  Values are those of dequant_rows_*_kernel
//                           (f32: the row; f16: widened; fp8: e4m3 x row scale), so the panel holds bit for bit what
//                           svs_index_debug_dequant returns for those rows.  Reads whole 16-byte chunks of a row per
//                           lane, as gather.h does, decoded by decode_chunk (chunk.h); the padding columns (>= d) are
//                           not copied.
//   drop_self_kernel        the search ran at count + 1; one wave per query removes the entry whose row is the source
//                           row (at most one: a search returns a row once), or the last entry when the source row is
//                           not among the count + 1 best, and writes `count` entries at stride `count`.
//
// Both are bandwidth trivia next to the score pass: a block of 1024 rows x 1536 halves is 3 MiB in, 6 MiB out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk.h"

namespace svs {

constexpr int NEIGHBORS_THREADS = 256;

// M: rows of ld16 16-byte chunks (DT: 0 f32, 1 f16, 2 fp8); list: nq local rows; out: [nq][d] f32.
// One work item = one 16-byte chunk of one listed row; chunks that lie wholly in the padding are not items.
template <int DT>
__global__ __launch_bounds__(NEIGHBORS_THREADS) void rows_as_queries_kernel(
    const u32x4* __restrict__ M, int ld16, const float* __restrict__ row_scales, const uint32_t* __restrict__ list,
    int nq, int d, float* __restrict__ out) {
  constexpr int EPC = elems_per_chunk(DT);
  const int used = (d + EPC - 1) / EPC;                    // chunks of a row that hold columns < d (<= ld16)
  const int64_t total = (int64_t)nq * used;
  const int64_t stride = (int64_t)gridDim.x * NEIGHBORS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * NEIGHBORS_THREADS + threadIdx.x; i < total; i += stride) {
    const int q = (int)(i / used);
    const int ch = (int)(i - (int64_t)q * used);
    const uint32_t row = list[q];
    float v[EPC];
    decode_chunk<DT>(M[(int64_t)row * ld16 + ch], v);
    if constexpr (DT == 2) {
      const float s = row_scales[row];
#pragma unroll
      for (int e = 0; e < EPC; ++e) v[e] = v[e] * s;
    }
    const int c0 = ch * EPC;
    float* o = out + (int64_t)q * d + c0;
    if ((d & 3) == 0 && c0 + EPC <= d) {   // (d % 4 == 0: every panel row, and c0, is 16-byte aligned)
#pragma unroll
      for (int e = 0; e < EPC; e += 4) *(v4f*)(o + e) = (v4f){v[e], v[e + 1], v[e + 2], v[e + 3]};
    } else {
#pragma unroll
      for (int e = 0; e < EPC; ++e)
        if (c0 + e < d) o[e] = v[e];
    }
  }
}

// in_s / in_r: [nq][count + 1] (a search's output); list: the nq local source rows; out_s / out_r: [nq][count].
// Entry i of the output is input entry i + (i >= p), p = the position of row_offset + list[q], or `count` if absent.
// A query marked by the fused path (in_r[0] == -2: its candidate list overflowed) keeps the mark in slot 0.
__global__ __launch_bounds__(NEIGHBORS_THREADS) void drop_self_kernel(
    const float* __restrict__ in_s, const int64_t* __restrict__ in_r, const uint32_t* __restrict__ list, int64_t row_offset,
    int nq, int count, float* __restrict__ out_s, int64_t* __restrict__ out_r) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (NEIGHBORS_THREADS / 64) + (threadIdx.x >> 6);
  if (q >= nq) return;   // (wave-uniform)
  const float* s = in_s + (int64_t)q * (count + 1);
  const int64_t* r = in_r + (int64_t)q * (count + 1);
  float* os = out_s + (int64_t)q * count;
  int64_t* orw = out_r + (int64_t)q * count;
  if (r[0] == -2) {
    if (lane == 0) orw[0] = -2;
    return;
  }
  const int64_t self = row_offset + (int64_t)list[q];
  int p = count;
  for (int i = lane; i <= count; i += 64)
    if (r[i] == self) p = i;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int o = __shfl_xor(p, off, 64);
    p = o < p ? o : p;
  }
  for (int i = lane; i < count; i += 64) {
    const int j = i + (i >= p ? 1 : 0);
    os[i] = s[j];
    orw[i] = r[j];
  }
}

}  // namespace svs

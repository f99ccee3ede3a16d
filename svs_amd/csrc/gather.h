// Score stage of a filtered search (svs_index_search_rows): nq queries against a LIST of rows, not the
// whole corpus.  scores[q][p] = <row list[p], query q> for p < m, stride sstride; the top-k stage
// (run_select) then ranks that compact vector like any other, and the host maps position p back to
// list[p] (the list is ascending, so "position desc" is "row desc").
//
// Roofline: HBM, bytes = m * row bytes per query group (4 B of list per row on top).  Unlike a corpus
// pass the rows are scattered, so what keeps the HBM busy is the number of independent row loads in
// flight: each wave loads its U row groups' list entries, then every 16-byte chunk of every row (12-16
// loads of 16 B per lane, i.e. 12-16 KiB per wave), before the first multiply.  Addresses are 64-bit
// (row * ld16 chunks): a 246 GB corpus has row offsets far past 2^32 bytes.
//
// Geometry per row length, as gemv_unrolled.h: T lanes share a row (T a power of two >= the row's
// 16-byte chunks, up to the wave), a wave instruction covers 64 / T rows, rows longer than a wave take
// NC chunks per lane; lanes past the row re-read its last chunk (in bounds) and drop what it adds.
//
// Arithmetic per dtype (that dtype's single-query kernel):
//   f32  f32 FMAs (DotF32)
//   f16  half rows x the half-rounded query, f32 accumulate (DotF16: v_dot2_f32_f16)
//   fp8  e4m3 rows decoded to f32 x the quantised query as f32, then (sum * row scale) * query scale, as
//        gemv_fp8_kernel.  The query chunk is stored packed (c->q8) and decoded here (DotFp8Packed): e4m3 -> f32
//        is exact, so these are the values stage_queries_fp8(want_f32 = true) would have written to c->q8f.
//
// Batches: G queries per workgroup (staged in LDS), each row read once per group.  A lane sums its chunks
// in chunk order, then seg_sum<T> -- the same for every G, so a query's scores are bit-identical whatever
// batch or group it was scored in.
//
// gather_wave is that lane-level body, one wave's rows against one query or a staged group; gather_scores_kernel here
// and gather_segments_kernel (segments.h) are prologues that decide which rows and which queries a wave takes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fp8.h"
#include "gemv_unrolled.h"

namespace svs {

constexpr int GATHER_G = 4;      // queries per workgroup when nq > 1 (LDS: 4 x row bytes, <= 64 KiB)
// waves per workgroup: 16, or 8 for rows of 12-16 chunks per lane (their 48-64 row VGPRs plus the query's need more
// than the 128 registers a 16-wave workgroup leaves a wave)
constexpr int gather_wpb(int nc) { return nc >= 12 ? 8 : 16; }

// DotFp8's arithmetic (the same FMAs on the same values, in the same order) with the query chunk kept PACKED and
// decoded next to the row bytes, as gemv_fp8_oneshot_kernel does: 4 registers per chunk instead of 16
struct DotFp8Packed {
  typedef u32x4 Q;
  __device__ __forceinline__ Q prep(u32x4 q) const { return q; }
  __device__ __forceinline__ float dot(u32x4 a, const Q& q, float acc) const {
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      float v[4], u[4];
      unpack_fp8x4(aw[w], v);
      unpack_fp8x4(qw[w], u);
      acc = fmaf(v[0], u[0], acc);
      acc = fmaf(v[1], u[1], acc);
      acc = fmaf(v[2], u[2], acc);
      acc = fmaf(v[3], u[3], acc);
    }
    return acc;
  }
};

template <int DT> struct GatherDot;
template <> struct GatherDot<0> { typedef DotF32 type; };
template <> struct GatherDot<1> { typedef DotF16 type; };
template <> struct GatherDot<2> { typedef DotFp8Packed type; };

// One wave of either gather kernel: rows list[0 .. nrows), 1 <= nrows <= (64 / T) * U, against the queries
// qsrc[g * ld16 ..] for g < (MANY ? gq : 1); scores[g * sstride + p] = <row list[p], query g>, q_scales[g] the
// query's scale (fp8).  Lanes past the rows re-read entry nrows - 1 and store nothing.  Everything a score's bits
// depend on -- the Dot type, the chunk order, seg_sum<T>, the fp8 scale order -- is here and nowhere else.
template <int DT, int T, int NC, int U, bool MANY>
__device__ __forceinline__ void gather_wave(const u32x4* __restrict__ M, int ld16, const uint32_t* __restrict__ list, int nrows,
                                            const u32x4* qsrc, int gq, const float* __restrict__ row_scales,
                                            const float* __restrict__ q_scales, float* __restrict__ scores, int64_t sstride) {
  typedef typename GatherDot<DT>::type Dot;
  constexpr bool SCALED = DT == 2;
  constexpr int RPW = 64 / T;
  const Dot dot{};
  const int lane = threadIdx.x & 63;
  const int sub = lane & (T - 1);
  const int rsub = lane / T;
  int col[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = sub + c * T;
    col[c] = i < ld16 ? i : ld16 - 1;
  }
  uint32_t row[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = u * RPW + rsub;
    row[u] = list[p < nrows ? p : nrows - 1];
  }
  u32x4 a[U][NC];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const u32x4* pr = M + (int64_t)row[u] * ld16;
#pragma unroll
    for (int c = 0; c < NC; ++c) a[u][c] = __builtin_nontemporal_load(pr + col[c]);
  }
  float rs[U];
#pragma unroll
  for (int u = 0; u < U; ++u) rs[u] = SCALED ? row_scales[row[u]] : 1.f;
  // (one query at a time: unrolled, the compiler would hold every query's chunks at once)
#pragma unroll 1
  for (int g = 0; g < (MANY ? gq : 1); ++g) {
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int i = sub + c * T;
      const typename Dot::Q qc = dot.prep(i < ld16 ? qsrc[(size_t)g * ld16 + i] : (u32x4){0u, 0u, 0u, 0u});
#pragma unroll
      for (int u = 0; u < U; ++u) {
        u32x4 av = a[u][c];
        // fp8: a row chunk's e4m3 -> f32 decode is the same for every query; hoisted out of this loop, or all
        // chunks decoded ahead of their FMAs, it would hold 16 registers per chunk instead of 4 and spill.  Empty
        // asm statements (kept in order) pin each chunk's decode between its own load and its FMAs.
        if constexpr (SCALED) asm volatile("" : "+v"(av));
        // (lanes past the row keep their sum: the chunk they re-read may hold inf or NaN, and 0 * inf is NaN)
        const float with_chunk = dot.dot(av, qc, acc[u]);
        acc[u] = i < ld16 ? with_chunk : acc[u];
        if constexpr (SCALED) asm volatile("" : "+v"(acc[u]));
      }
    }
    float* out = scores + (size_t)g * sstride;
    const float sq = SCALED ? q_scales[g] : 1.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float v = seg_sum<T>(acc[u]);
      if constexpr (SCALED) v = v * rs[u] * sq;
      const int p = u * RPW + rsub;
      if (sub == 0 && p < nrows) out[p] = v;
    }
  }
}

// M: rows of ld16 16-byte chunks; list: m local rows; q: nq staged queries of ld16 chunks each (zero padded
// like the rows); row_scales / q_scales: fp8 only.  Grid: (row blocks, query groups); a wave takes (64 / T) U rows.
template <int DT, int T, int NC, int U, int G>
__global__ __launch_bounds__(gather_wpb(NC) * 64) void gather_scores_kernel(
    const u32x4* __restrict__ M, int ld16, const uint32_t* __restrict__ list, int64_t m,
    const u32x4* __restrict__ q, int nq, const float* __restrict__ row_scales, const float* __restrict__ q_scales,
    float* __restrict__ scores, int64_t sstride) {
  constexpr int W = 64 / T * U, WPB = gather_wpb(NC);
  const int q0 = blockIdx.y * G;
  const int gq = nq - q0 < G ? nq - q0 : G;   // queries of this group (block-uniform)
  q += (size_t)q0 * ld16;
  const u32x4* qsrc = q;
  if constexpr (G > 1) {
    extern __shared__ u32x4 q_lds[];   // [gq][ld16]
    for (int i = threadIdx.x; i < gq * ld16; i += WPB * 64) q_lds[i] = q[i];
    __syncthreads();
    qsrc = q_lds;
  }
  const int64_t base = ((int64_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * W;
  if (base >= m) return;
  const int nrows = m - base < W ? (int)(m - base) : W;
  gather_wave<DT, T, NC, U, (G > 1)>(M, ld16, list + base, nrows, qsrc, gq, row_scales, q_scales + q0,
                                     scores + (size_t)q0 * sstride + base, sstride);
}

}  // namespace svs

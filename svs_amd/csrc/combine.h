// Combined search (svs_index_search_combined): rows ranked by how they score against m vectors at once.
//
// Definition (include/svs_amd.h).  s_j[i] is the f32 score the index's single-query kernel gives row i for vector j
// (what svs_index_scores_n returns).  The term t_j = w_j * s_j is ONE f32 multiplication, and
//     MAX   key_score(max_j score_key(t_j))      MIN   key_score(min_j score_key(t_j))      (keys.h: the order's key)
//     SUM   ((t_0 + t_1) + t_2) + ...            f32 additions in vector order, never contracted with the multiplication
// There is ONE implementation of that: combine_init / combine_step / combine_finish below.  Both routes call it:
//
//   fused     combine_f32_kernel / combine_f16_kernel / combine_fp8_kernel: the one-shot geometry of the dtype's
//             single-query kernel (grid, R rows per wave, WPB waves).  A wave loads its R rows ONCE (nontemporal), then
//             streams the m vectors through them, each with the arithmetic of a pass of its own (row_dot_f32,
//             row_dot_f16 behind round_query8, row_dot_fp8 times the row's and the vector's scale), folds each score
//             into the row's accumulator and stores one float per row.
//   passes    m launches of the route's own single-query kernel into m score vectors, then combine_scores_kernel:
//             elementwise over the m vectors, 16 bytes per lane, the combined vector written over vector 0.
//
// Where the fused kernels keep the vectors: NOT in LDS.  Every wave reads vector j's slice from global memory at the
// top of iteration j (m * ld * 4 bytes, at most 128 KB at m = 8 and 4096 floats: resident in L2 after the first
// workgroups, as gemv_f32_oneshot_kernel<..., QLDS = false> reads its one query).  m * ld * 4 bytes of LDS would be
// 48 KB at m = 8, d = 1536 and take the second 16-wave workgroup off the CU; the kernels use no LDS at all, so their
// occupancy is their registers': the rows (R * NSTEP chunks) plus ONE vector's slice (NSTEP chunks), whatever m.
// m, the op and the weights are wave-uniform (kernel arguments and scalar loads): no divergent control flow over them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp8.h"
#include "gemv_f16.h"
#include "gemv_f32.h"
#include "keys.h"

namespace svs {

constexpr int CB_MAX = 0, CB_MIN = 1, CB_SUM = 2;   // SVS_COMBINE_MAX / _MIN / _SUM
constexpr int CB_MAX_VECTORS = 8;                   // SVS_COMBINE_MAX_VECTORS

// ---- the definition -----------------------------------------------------------------------------------------------
// The accumulator is 32 bits: the running key (MAX, MIN) or the running sum's bits (SUM).  Start values: the key below
// every score's (-inf has key 0x007fffff), the key above every score's but NaN's own (a NaN term IS that key), and
// -0.0f, the one f32 that x + (-0.0f) gives back x for every x, -0.0f and +0.0f included.
__device__ __forceinline__ uint32_t combine_init(int op) { return op == CB_MAX ? 0u : (op == CB_MIN ? 0xffffffffu : 0x80000000u); }
// One vector's score s under its weight w folded in.  The multiplication and the addition are two roundings: this
// block is compiled with contraction off, so that no v_fma / v_fmac joins them.
__device__ __forceinline__ uint32_t combine_step(uint32_t acc, float s, float w, int op) {
#pragma clang fp contract(off)
  const float t = w * s;
  if (op == CB_SUM) {
    const float sum = bits_f32(acc) + t;
    return f32_bits(sum);
  }
  const uint32_t k = score_key(t);
  return op == CB_MAX ? (k > acc ? k : acc) : (k < acc ? k : acc);
}
__device__ __forceinline__ float combine_finish(uint32_t acc, int op) { return op == CB_SUM ? bits_f32(acc) : key_score(acc); }

// ---- passes route: vectors[j] = scores + j * sstride (j < m), combined into vectors[0] ------------------------------
// n4 = sstride / 4 groups of four rows (the allocation is padded to a multiple of 4; the padding's values are never read
// by anyone).  Each lane reads its group of every vector before it writes the group of vector 0.
__global__ __launch_bounds__(256) void combine_scores_kernel(float* __restrict__ scores, int64_t sstride, int64_t n4, int m,
                                                             const float* __restrict__ weights, int op) {
  v4f* s4 = (v4f*)scores;
  const int64_t stride4 = sstride >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t a0 = combine_init(op), a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
      const v4f s = s4[j * stride4 + i];
      const float w = weights[j];
      a0 = combine_step(a0, s.x, w, op);
      a1 = combine_step(a1, s.y, w, op);
      a2 = combine_step(a2, s.z, w, op);
      a3 = combine_step(a3, s.w, w, op);
    }
    s4[i] = (v4f){combine_finish(a0, op), combine_finish(a1, op), combine_finish(a2, op), combine_finish(a3, op)};
  }
}

// ---- fused route ------------------------------------------------------------------------------------------------------
// Common to the three: workgroup b owns rows [b * WPB * R, (b + 1) * WPB * R), wave w of it R consecutive rows; a wave
// past the last row leaves at once (no barrier anywhere); rows past n are clamped to the last row and their result is
// not stored; lane r < R stores row0 + r.  The f32 and fp8 row loads are spelled in every kernel: lifted into helpers
// like load_rows_f16 they changed the scalar address code of 26 f32 and 4 fp8 instantiations (both families).

// f32, ld == NSTEP * 256 floats.  q: the m vectors as the single-query kernel reads one, [m][ld] floats, 16-byte aligned.
template <int NSTEP, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void combine_f32_kernel(const v4f* __restrict__ M, const v4f* __restrict__ q,
                                                               const float* __restrict__ weights, int m, int op,
                                                               float* __restrict__ out, int64_t n) {
  constexpr int LD4 = NSTEP * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  v4f buf[R][NSTEP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const v4f* p = M + row * LD4 + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = ldg4<true>(p + j * 64);
  }
  uint32_t acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = combine_init(op);
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    v4f qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = q[t * LD4 + j * 64 + lane];
    const float w = weights[t];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = combine_step(acc[r], row_dot_f32<NSTEP>(buf[r], qv), w, op);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) res = lane == r ? combine_finish(acc[r], op) : res;
  const int64_t row = row0 + lane;
  if (lane < R && row < n) out[row] = res;
}

// One half row against one rounded vector: the chain of score_rows_f16 (gemv_f16.h) -- dot8 into s0 (even j) and s1
// (odd j), then wave_sum(s0 + s1).  Spelled again here, not lifted out of gemv_f16.h: calling a helper from
// gemv_f16_oneshot_kernel changed the register allocation of the kernel every screened f32 search runs.
template <int NSTEP>
__device__ __forceinline__ float row_dot_f16(const u32x4 (&row)[NSTEP], const u32x4 (&qv)[NSTEP]) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < NSTEP; ++j) {
    if (j & 1) s1 = dot8(row[j], qv[j], s1);
    else s0 = dot8(row[j], qv[j], s0);
  }
  return wave_sum(s0 + s1);
}

// f16, ld16 == NSTEP * 512 halves.  q: [m][ld16] floats; each wave rounds the slice it is about to use (round_query8).
template <int NSTEP, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void combine_f16_kernel(const u32x4* __restrict__ M, const v4f* __restrict__ q,
                                                               const float* __restrict__ weights, int m, int op,
                                                               float* __restrict__ out, int64_t n) {
  constexpr int LD8 = NSTEP * 64;   // row stride in 16-byte units; a vector is 2 * LD8 v4f
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  u32x4 buf[R][NSTEP];
  load_rows_f16<NSTEP, R>(buf, M, row0, n, lane);
  uint32_t acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = combine_init(op);
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    const v4f* qt = q + (int64_t)t * (2 * LD8);
    u32x4 qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = round_query8(qt[(j * 64 + lane) * 2], qt[(j * 64 + lane) * 2 + 1]);
    const float w = weights[t];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = combine_step(acc[r], row_dot_f16<NSTEP>(buf[r], qv), w, op);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) res = lane == r ? combine_finish(acc[r], op) : res;
  const int64_t row = row0 + lane;
  if (lane < R && row < n) out[row] = res;
}

// fp8, ld8 == NSTEP * 64 * LB bytes.  q8: the m vectors quantised one by one as a query is, [m][ld8] bytes, with their
// scales q_scales[m].  A score is wave_sum(...) * row scale * vector scale, multiplied in that order.
// (The compiler keeps the row bytes CONVERTED to f32 across the loop over the vectors: 78-104 registers for all but the
//  512-byte rows, against the single-query kernel's 58-66, so one 16-wave workgroup per CU, not two.  No scratch; the
//  conversions are paid once per row instead of once per vector.)
template <int NSTEP, int LB, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void combine_fp8_kernel(const uint8_t* __restrict__ M, const float* __restrict__ row_scales,
                                                               const uint8_t* __restrict__ q8, const float* __restrict__ q_scales,
                                                               const float* __restrict__ weights, int m, int op,
                                                               float* __restrict__ out, int64_t n) {
  typedef typename Fp8Chunk<LB>::type chunk_t;
  constexpr int64_t LDB = (int64_t)NSTEP * 64 * LB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  chunk_t buf[R][NSTEP];
  float rs[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const chunk_t* p = (const chunk_t*)(M + row * LDB) + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = __builtin_nontemporal_load(p + j * 64);
    rs[r] = row_scales[row];
  }
  uint32_t acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = combine_init(op);
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    const chunk_t* qt = (const chunk_t*)(q8 + (int64_t)t * LDB);
    chunk_t qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = qt[j * 64 + lane];
    const float sq = q_scales[t], w = weights[t];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = combine_step(acc[r], row_dot_fp8<NSTEP, LB>(buf[r], qv) * rs[r] * sq, w, op);
  }
  float res = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) res = lane == r ? combine_finish(acc[r], op) : res;
  const int64_t row = row0 + lane;
  if (lane < R && row < n) out[row] = res;
}

// ---- multi-score pass (svs_index_search_collapsed_combined, collapse_combine.h) ------------------------------------------
// The three fused kernels again, with one difference: vector t's score of row row0 + r is not folded, it is STORED, to
// out[t * sstride + row] -- m score vectors, each with the bits of a single-query pass of its own.  The geometry, the
// loads and the arithmetic are the combine kernels'; no weights, no op.  Kernels of their own, not a template flag on
// the ones above: those keep their names and their register allocation.  No LDS, no scratch: the rows plus one
// vector's slice, as above; lane r < R stores one float per vector (m * R dwords per wave against R rows loaded).
template <int NSTEP, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void multi_score_f32_kernel(const v4f* __restrict__ M, const v4f* __restrict__ q, int m,
                                                                   float* __restrict__ out, int64_t sstride, int64_t n) {
  constexpr int LD4 = NSTEP * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  v4f buf[R][NSTEP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const v4f* p = M + row * LD4 + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = ldg4<true>(p + j * 64);
  }
  const int64_t row = row0 + lane;
  const bool writer = lane < R && row < n;
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    v4f qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = q[t * LD4 + j * 64 + lane];
    float res = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float s = row_dot_f32<NSTEP>(buf[r], qv);
      res = lane == r ? s : res;
    }
    if (writer) out[(int64_t)t * sstride + row] = res;
  }
}

template <int NSTEP, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void multi_score_f16_kernel(const u32x4* __restrict__ M, const v4f* __restrict__ q, int m,
                                                                   float* __restrict__ out, int64_t sstride, int64_t n) {
  constexpr int LD8 = NSTEP * 64;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  u32x4 buf[R][NSTEP];
  load_rows_f16<NSTEP, R>(buf, M, row0, n, lane);
  const int64_t row = row0 + lane;
  const bool writer = lane < R && row < n;
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    const v4f* qt = q + (int64_t)t * (2 * LD8);
    u32x4 qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = round_query8(qt[(j * 64 + lane) * 2], qt[(j * 64 + lane) * 2 + 1]);
    float res = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float s = row_dot_f16<NSTEP>(buf[r], qv);
      res = lane == r ? s : res;
    }
    if (writer) out[(int64_t)t * sstride + row] = res;
  }
}

template <int NSTEP, int LB, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void multi_score_fp8_kernel(const uint8_t* __restrict__ M, const float* __restrict__ row_scales,
                                                                   const uint8_t* __restrict__ q8, const float* __restrict__ q_scales, int m,
                                                                   float* __restrict__ out, int64_t sstride, int64_t n) {
  typedef typename Fp8Chunk<LB>::type chunk_t;
  constexpr int64_t LDB = (int64_t)NSTEP * 64 * LB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  chunk_t buf[R][NSTEP];
  float rs[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const chunk_t* p = (const chunk_t*)(M + row * LDB) + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = __builtin_nontemporal_load(p + j * 64);
    rs[r] = row_scales[row];
  }
  const int64_t row = row0 + lane;
  const bool writer = lane < R && row < n;
#pragma unroll 1
  for (int t = 0; t < m; ++t) {
    const chunk_t* qt = (const chunk_t*)(q8 + (int64_t)t * LDB);
    chunk_t qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = qt[j * 64 + lane];
    const float sq = q_scales[t];
    float res = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float s = row_dot_fp8<NSTEP, LB>(buf[r], qv) * rs[r] * sq;
      res = lane == r ? s : res;
    }
    if (writer) out[(int64_t)t * sstride + row] = res;
  }
}

}  // namespace svs

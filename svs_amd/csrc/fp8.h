// fp8-resident corpus (SVS_DTYPE_FP8; BASELINE.json configs[4]: 10M x 3072).
// OCP e4m3fn (gfx950's native fp8, NOT the MI300 fnuz encoding) with one f32
// scale per row: unit-norm rows have |x| ~ 1/sqrt(d) ~ 0.02, at the very bottom
// of e4m3's normal range (2^-6), so each row is scaled to put its largest
// magnitude on 448 (the e4m3 maximum) before rounding (RNE):
//     scale_i = max(max_d |M[i,d]|, 7 * 2^-120) / 448        q8[i,d] = e4m3(M[i,d] * (1 / scale_i))
// (the maximum skips NaN elements; a row whose maximum is 0 gets scale 1).  The floor under the maximum keeps the
// scale at or above 2^-126, so that 1 / scale_i is finite for every finite row: without it a row with
// 0 < max|x| < 448 / FLT_MAX had 1 / scale = inf and was stored as NaN throughout.  Elements of a row below the floor
// quantise against the floor, the smallest of them to zero; every row at or above it stores what it did without it.
// A row with an infinite element has scale inf and reads back as NaN.
// Queries are quantised the same way.  A score is
//     scale_i * scale_q * sum_d f32(q8[i,d]) * f32(q8q[d])      (f32 accumulate)
// and the parity oracle for this dtype is numpy's f32 path on the DEQUANTISED
// corpus and query (svs_index_debug_dequant returns exactly what is stored).
// Recall against the f32 corpus is a property of the rounding, reported separately.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemv_f32.h"

namespace svs {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr float FP8_MAX = 448.0f;
constexpr float FP8_MIN_ROW_MAX = 0x1.cp-118f;   // 7 * 2^-120: FP8_MIN_ROW_MAX / FP8_MAX = 2^-126, the smallest scale

// 4 floats -> 4 packed e4m3 bytes (RNE)
__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
  int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
  return (uint32_t)p;
}
__device__ __forceinline__ void unpack_fp8x4(uint32_t p, float (&o)[4]) {
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)p, false);
  const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)p, true);
  o[0] = lo.x; o[1] = lo.y; o[2] = hi.x; o[3] = hi.y;
}

// One wave per row: f32 row (stride src_ld) -> e4m3 row (stride ld8 bytes, zero
// padded) + scale.  Optionally also the quantised values back as f32 (qf, stride
// ld8 floats): the single-query kernel reads the query that way.
__global__ __launch_bounds__(256) void quantize_rows_fp8_kernel(
    const float* __restrict__ src, int64_t n, int d, int64_t src_ld, uint8_t* __restrict__ dst, int ld8,
    float* __restrict__ scales, float* __restrict__ qf) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t W = (int64_t)gridDim.x * 4;
  for (int64_t row = gw; row < n; row += W) {
    const float* s = src + row * src_ld;
    float mx = 0.f;
    for (int c = lane; c < d; c += 64) mx = fmaxf(mx, fabsf(s[c]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    const float scale = mx > 0.f ? fmaxf(mx, FP8_MIN_ROW_MAX) / FP8_MAX : 1.0f;
    const float inv = 1.0f / scale;
    if (lane == 0) scales[row] = scale;
    uint32_t* o = (uint32_t*)(dst + row * ld8);
    for (int c4 = lane; c4 < ld8 / 4; c4 += 64) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c4 * 4 + e;
        v[e] = c < d ? s[c] * inv : 0.f;
      }
      const uint32_t p = pack_fp8x4(v[0], v[1], v[2], v[3]);
      o[c4] = p;
      if (qf) {
        float b[4];
        unpack_fp8x4(p, b);
        float* q = qf + row * ld8 + c4 * 4;
        q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; q[3] = b[3];
      }
    }
  }
}

// debug / parity: stored rows back as f32 (value * scale), out stride d
__global__ void dequant_rows_fp8_kernel(const uint8_t* __restrict__ rows, const float* __restrict__ scales,
                                        int64_t row0, int64_t nrows, int d, int ld8, float* __restrict__ out) {
  const int64_t total = nrows * d;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / d;
    const int c = (int)(i - r * d);
    const uint8_t b = rows[(row0 + r) * ld8 + c];
    out[i] = __builtin_amdgcn_cvt_f32_fp8((int)b, 0) * scales[row0 + r];
  }
}

// 16 e4m3 bytes (one 16-byte load) times 16 f32 query values
__device__ __forceinline__ float dot16_fp8(u32x4_t a, const v4f* q, float acc) {
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t p = w == 0 ? a.x : (w == 1 ? a.y : (w == 2 ? a.z : a.w));
    float v[4];
    unpack_fp8x4(p, v);
    const v4f qq = q[w];
    acc = fmaf(v[0], qq.x, acc);
    acc = fmaf(v[1], qq.y, acc);
    acc = fmaf(v[2], qq.z, acc);
    acc = fmaf(v[3], qq.w, acc);
  }
  return acc;
}

// ---- single query, hot kernel: one-shot grid, R rows per wave (gemv_f32.h geometry)
// A row of ld8 = NSTEP * 64 * LB bytes is NSTEP wave-wide loads of LB (16 or 8)
// bytes per lane.
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

template <int LB> struct Fp8Chunk;
template <> struct Fp8Chunk<16> { typedef u32x4_t type; };
template <> struct Fp8Chunk<8> { typedef u32x2_t type; };

// One row against one packed query: THE summation order of the one-shot row lengths.  Lane l holds chunk j * 64 + l of
// the row and of the query; the 32-bit words of a chunk alternate between s0 (even) and s1 (odd); then wave_sum(s0 + s1),
// still unscaled.  gemv_fp8_oneshot_kernel and the combined search's fused kernel (combine.h) both call this.
template <int NSTEP, int LB>
__device__ __forceinline__ float row_dot_fp8(const typename Fp8Chunk<LB>::type (&row)[NSTEP], const typename Fp8Chunk<LB>::type (&qv)[NSTEP]) {
  constexpr int NW = LB / 4;               // 32-bit words per lane per load
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < NSTEP; ++j) {
    uint32_t aw[NW], qw[NW];
    if constexpr (NW == 4) {
      aw[0] = row[j].x; aw[1] = row[j].y; aw[2] = row[j].z; aw[3] = row[j].w;
      qw[0] = qv[j].x; qw[1] = qv[j].y; qw[2] = qv[j].z; qw[3] = qv[j].w;
    } else {
      aw[0] = row[j].x; aw[1] = row[j].y;
      qw[0] = qv[j].x; qw[1] = qv[j].y;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      float v[4], u[4];
      unpack_fp8x4(aw[w], v);
      unpack_fp8x4(qw[w], u);
      float& acc = (w & 1) ? s1 : s0;
      acc = fmaf(v[0], u[0], acc);
      acc = fmaf(v[1], u[1], acc);
      acc = fmaf(v[2], u[2], acc);
      acc = fmaf(v[3], u[3], acc);
    }
  }
  return wave_sum(s0 + s1);
}

// The query stays PACKED (e4m3, LB bytes per lane per step) and is converted next
// to the row bytes: 4x fewer registers than holding it as f32, which is what lets
// two 16-wave workgroups share a CU (the kernel is HBM-bound; the extra
// v_cvt_pk_f32_fp8 are free).
template <int NSTEP, int LB, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void gemv_fp8_oneshot_kernel(
    const uint8_t* __restrict__ M, const float* __restrict__ row_scales, const uint8_t* __restrict__ q8,
    const float* __restrict__ q_scale, float* __restrict__ scores, int64_t n) {
  typedef typename Fp8Chunk<LB>::type chunk_t;
  constexpr int64_t LDB = (int64_t)NSTEP * 64 * LB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
  if (row0 >= n) return;
  chunk_t buf[R][NSTEP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const chunk_t* p = (const chunk_t*)(M + row * LDB) + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = __builtin_nontemporal_load(p + j * 64);
  }
  chunk_t qv[NSTEP];
#pragma unroll
  for (int j = 0; j < NSTEP; ++j) qv[j] = ((const chunk_t*)q8)[j * 64 + lane];
  const float sq = q_scale[0];
  float out = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const float v = row_dot_fp8<NSTEP, LB>(buf[r], qv) * row_scales[row] * sq;
    out = lane == r ? v : out;
  }
  const int64_t row = row0 + lane;
  if (lane < R && row < n) scores[row] = out;
}

// ---- single query: T lanes per row, 64/T rows per wave step --------------------
// M: e4m3 rows (ld8 bytes, multiple of 16); qf: the quantised query as f32 (ld8
// floats, zero padded); score = row scale * query scale * dot.
template <int T>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(
    const u32x4_t* __restrict__ M, const float* __restrict__ row_scales, const v4f* __restrict__ qf,
    const float* __restrict__ q_scale, float* __restrict__ scores, int64_t n, int ld16) {
  constexpr int RPW = 64 / T;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (T - 1);
  const int rsub = lane / T;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t W = (int64_t)gridDim.x * 4;
  const float sq = q_scale[0];
  for (int64_t base = gw * RPW; base < n; base += W * RPW) {
    int64_t row = base + rsub;
    const bool live = row < n;
    row = live ? row : n - 1;
    const u32x4_t* p = M + row * ld16;
    float acc = 0.f;
    for (int c = sub; c < ld16; c += T) acc = dot16_fp8(__builtin_nontemporal_load(p + c), qf + c * 4, acc);
#pragma unroll
    for (int off = T / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (sub == 0 && live) scores[row] = acc * row_scales[row] * sq;
  }
}

}  // namespace svs

// f16-resident corpus (SVS_DTYPE_F16; BASELINE.json configs[2]/[3]): rows are
// rounded to IEEE half (RNE) once at upload, halving the HBM bytes per query
// (3.07 GB at 1M x 1536).  Queries are rounded to half as well, so every score is
//     sum_d f32(half(M[i,d])) * f32(half(q[d]))     accumulated in f32
// -- products of two halves are exact in f32 -- and the oracle for this dtype is
// numpy's f32 path on the dequantised corpus and query.
// Recall against the f32 corpus is a property of the rounding, not of the kernel.
//
// Single-query score kernel: same one-shot geometry as gemv_f32.h (HBM-bound,
// algorithmic bytes = n * ld * 2).  A row of ld = NSTEP*512 halves is NSTEP
// wave-wide 1 KiB loads (8 halves per lane); the query sits in NSTEP*4 packed
// half2 registers per lane; v_dot2_f32_f16 does two multiply-adds per lane-op.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "gemv_f32.h"
#include "pass_share.h"

namespace svs {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef v4f __attribute__((address_space(1))) global_v4f;

// 8 halves x 8 halves + acc (four v_dot2_f32_f16).  The operands are split with
// shufflevector on the half view: element-indexing the u32 view and bit-casting
// each element made hipcc (ROCm 7.2) reuse element 0 four times.
__device__ __forceinline__ float dot8(u32x4 a, u32x4 b, float acc) {
  const h8 x = __builtin_bit_cast(h8, a), y = __builtin_bit_cast(h8, b);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(x, x, 0, 1), __builtin_shufflevector(y, y, 0, 1), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(x, x, 2, 3), __builtin_shufflevector(y, y, 2, 3), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(x, x, 4, 5), __builtin_shufflevector(y, y, 4, 5), acc, false);
  acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(x, x, 6, 7), __builtin_shufflevector(y, y, 6, 7), acc, false);
  return acc;
}

// f32 rows (stride src_ld) -> half rows (stride ld16, zero padded).  grid-stride.
__global__ void convert_rows_f16_kernel(const float* __restrict__ src, int64_t n, int d, int64_t src_ld,
                                        _Float16* __restrict__ dst, int ld16) {
  const int64_t total = n * ld16;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / ld16;
    const int c = (int)(i - r * ld16);
    dst[i] = c < d ? (_Float16)src[r * src_ld + c] : (_Float16)0.f;
  }
}

// debug / parity: half rows back as f32, out stride d
__global__ void dequant_rows_f16_kernel(const _Float16* __restrict__ rows, int64_t row0, int64_t nrows, int d,
                                        int ld16, float* __restrict__ out) {
  const int64_t total = nrows * d;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / d;
    out[i] = (float)rows[(row0 + r) * ld16 + (i - r * d)];
  }
}

// queries f32 [nq][d] -> half [nq][ld16] zero padded (tiny)
__global__ void convert_queries_f16_kernel(const float* __restrict__ q, int nq, int d,
                                           _Float16* __restrict__ dst, int ld16) {
  const int total = nq * ld16;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / ld16, c = i - r * ld16;
    dst[i] = c < d ? (_Float16)q[(int64_t)r * d + c] : (_Float16)0.f;
  }
}

// ---- hot kernel: ld16 == NSTEP * 512 halves, one-shot grid, R rows per wave ----
// q is the f32 query (d = ld16 floats, 16-byte aligned): each wave rounds its
// slice to half itself (RNE), saving a conversion launch on the latency path.
//
// plan != nullptr (run-ahead pipeline, pass_share.h): the pass serves the plan's c queries from ONE load of its
// rows -- the rows stay in registers and the queries are streamed through them one after another, each with the
// arithmetic of a pass of its own (same dot8 chain, same wave_sum), each into its own score vector.  c is
// wave-uniform (a scalar load); c == 0 returns before the first row load.  plan == nullptr: q and scores, as ever.
//
// Under a plan the queries are rounded ONCE PER WORKGROUP: the waves share the c * NSTEP 1 KiB slices (f32 in, the
// same (_Float16) conversion, halves out) among themselves, store them into dynamic LDS (c * NSTEP KiB; the launch
// gives share_limit * ld16 * 2 bytes) and meet at one barrier; the loop over the queries then reads its qv[j] as one
// 16-byte LDS word per lane (consecutive lanes, consecutive words: no bank conflicts).  The query loads are issued
// in front of the row loads and the rows stay in flight across the fill and the barrier.  Every wave of the
// workgroup takes part in the fill, also those of the tail workgroup that have no row; they leave behind the barrier.
//
// The plan branch walks the row blocks blk = blockIdx.x, blockIdx.x + gridDim.x, ...: the one-shot grid makes one
// trip; a search the host expects an earlier pass to serve is launched on a thin grid (one resident set of
// workgroups), which returns at c == 0 and otherwise strides over all blocks -- the same scores, only slower.
//
// Row lengths on which the plan is compiled in: those where the loop over the plan's queries keeps the kernel at its
// occupancy without scratch (the build's resource report: 512 .. 3584 halves; at 4096 the loop costs 10 registers and
// two waves per SIMD).  Elsewhere the kernel ignores `plan`, and the host never passes one.
constexpr int F16_SHARE_NSTEP_MAX = 7;
constexpr bool f16_rows_share(int nstep) { return nstep >= 1 && nstep <= F16_SHARE_NSTEP_MAX; }

// eight f32 of a query -> eight halves (RNE), packed as the rows are
__device__ __forceinline__ u32x4 round_query8(v4f lo, v4f hi) {
  const h2 p0 = {(_Float16)lo.x, (_Float16)lo.y}, p1 = {(_Float16)lo.z, (_Float16)lo.w};
  const h2 p2 = {(_Float16)hi.x, (_Float16)hi.y}, p3 = {(_Float16)hi.z, (_Float16)hi.w};
  return (u32x4){__builtin_bit_cast(uint32_t, p0), __builtin_bit_cast(uint32_t, p1),
                 __builtin_bit_cast(uint32_t, p2), __builtin_bit_cast(uint32_t, p3)};
}

template <int NSTEP, int R>
__device__ __forceinline__ void load_rows_f16(u32x4 (&buf)[R][NSTEP], const u32x4* __restrict__ M, int64_t row0, int64_t n, int lane) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int64_t row = row0 + r;
    row = row < n ? row : n - 1;
    const u32x4* p = M + row * (NSTEP * 64) + lane;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) buf[r][j] = __builtin_nontemporal_load(p + j * 64);
  }
}

// one query over the wave's R rows: lane r < R stores the score of row0 + r
template <int NSTEP, int R>
__device__ __forceinline__ void score_rows_f16(const u32x4 (&buf)[R][NSTEP], const u32x4 (&qv)[NSTEP], float* __restrict__ st,
                                               int64_t row0, int64_t n, int lane) {
  float out = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) {
      if (j & 1) s1 = dot8(buf[r][j], qv[j], s1);
      else s0 = dot8(buf[r][j], qv[j], s0);
    }
    const float v = wave_sum(s0 + s1);
    out = lane == r ? v : out;
  }
  const int64_t row = row0 + lane;
  if (lane < R && row < n) st[row] = out;
}

template <int NSTEP, int R, int WPB>
__global__ __launch_bounds__(WPB * 64) void gemv_f16_oneshot_kernel(
    const u32x4* __restrict__ M, const v4f* __restrict__ q, float* __restrict__ scores, int64_t n,
    const PassPlan* __restrict__ plan_arg) {
  const PassPlan* __restrict__ plan = f16_rows_share(NSTEP) ? plan_arg : nullptr;
  constexpr int LD4 = NSTEP * 64;  // row stride in 16-byte units
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (!plan) {   // (the kernel as it was before plans: NSTEP > F16_SHARE_NSTEP_MAX compiles to exactly this)
    const int64_t row0 = ((int64_t)blockIdx.x * WPB + wave) * R;
    if (row0 >= n) return;
    u32x4 buf[R][NSTEP];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int64_t row = row0 + r;
      row = row < n ? row : n - 1;
      const u32x4* p = M + row * LD4 + lane;
#pragma unroll
      for (int j = 0; j < NSTEP; ++j) buf[r][j] = __builtin_nontemporal_load(p + j * 64);
    }
    u32x4 qv[NSTEP];
#pragma unroll
    for (int j = 0; j < NSTEP; ++j) qv[j] = round_query8(q[(j * 64 + lane) * 2], q[(j * 64 + lane) * 2 + 1]);
    float out = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int j = 0; j < NSTEP; ++j) {
        if (j & 1) s1 = dot8(buf[r][j], qv[j], s1);
        else s0 = dot8(buf[r][j], qv[j], s0);
      }
      const float v = wave_sum(s0 + s1);
      out = lane == r ? v : out;
    }
    const int64_t row = row0 + lane;
    if (lane < R && row < n) scores[row] = out;
    return;
  }
  u32x4 buf[R][NSTEP];
  u32x4 qv[NSTEP];
  extern __shared__ u32x4 plan_q16[];   // [c][NSTEP][64]: the plan's queries as halves
  const int c = __builtin_amdgcn_readfirstlane((int)plan->c);
  if (c == 0) return;
  // this wave's share of the fill: slices s = wave, wave + WPB, ... of the c * NSTEP (query t = s / NSTEP, step s % NSTEP)
  constexpr int FILL = (SHARE_MAX * NSTEP + WPB - 1) / WPB;
  v4f lo[FILL], hi[FILL];
#pragma unroll
  for (int f = 0; f < FILL; ++f) {
    const int s = wave + f * WPB;
    if (s < c * NSTEP) {
      // (a global-memory pointer, said so: loaded from the plan it would be a flat one, whose loads the rows behind
      //  them could not stay in flight across)
      const global_v4f* qs = (const global_v4f*)(plan->q[s / NSTEP] + ((s % NSTEP) * 64 + lane) * 2);
      lo[f] = qs[0];
      hi[f] = qs[1];
    }
  }
  const int64_t nblk = (n + R * WPB - 1) / (R * WPB);
  int64_t blk = blockIdx.x;
  int64_t row0 = (blk * WPB + wave) * R;
  bool live = row0 < n;
  // (no branch around the first row loads -- a wave without rows loads the clamped last row -- so that the wait in
  //  front of the rounding counts them and lets them stay in flight)
  load_rows_f16<NSTEP, R>(buf, M, row0, n, lane);
#pragma unroll
  for (int f = 0; f < FILL; ++f) {
    const int s = wave + f * WPB;
    if (s < c * NSTEP) plan_q16[s * 64 + lane] = round_query8(lo[f], hi[f]);
  }
  __syncthreads();
  while (live) {
#pragma unroll 1
    for (int t = 0; t < c; ++t) {
#pragma unroll
      for (int j = 0; j < NSTEP; ++j) qv[j] = plan_q16[(t * NSTEP + j) * 64 + lane];
      score_rows_f16<NSTEP, R>(buf, qv, plan->scores[t], row0, n, lane);
    }
    blk += gridDim.x;
    row0 = (blk * WPB + wave) * R;
    live = blk < nblk && row0 < n;
    if (live) load_rows_f16<NSTEP, R>(buf, M, row0, n, lane);
  }
}

// ---- generic kernel: any d (rows zero padded to ld16 % 8 == 0) ----------------
template <int T>
__global__ __launch_bounds__(256) void gemv_f16_generic_kernel(
    const u32x4* __restrict__ M, const u32x4* __restrict__ q, float* __restrict__ scores, int64_t n,
    int ld8) {
  constexpr int RPW = 64 / T;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (T - 1);
  const int rsub = lane / T;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t W = (int64_t)gridDim.x * 4;
  for (int64_t base = gw * RPW; base < n; base += W * RPW) {
    int64_t row = base + rsub;
    const bool live = row < n;
    row = live ? row : n - 1;
    const u32x4* p = M + row * ld8;
    float acc = 0.f;
    for (int c = sub; c < ld8; c += T) acc = dot8(p[c], q[c], acc);
#pragma unroll
    for (int off = T / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (sub == 0 && live) scores[row] = acc;
  }
}

}  // namespace svs

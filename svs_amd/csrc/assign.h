// Nearest-vector assignment (svs_index_assign): for every stored row of a range, which of c caller-given vectors it
// scores best against -- the transposed question of a search.  The c vectors are ingested per call into a small device
// image in the index's own storage format (at most 1024 rows: it stays in L2 / Infinity Cache); the corpus rows are
// streamed past it once per sweep.
//
// One launch on the context's stream:
//
//   assign_rows_kernel<DT, NA>  Workgroups stride over tiles of AS_ROWS = 64 CONSECUTIVE corpus rows (no gather list, 64-bit
//                            addressing row * ld16).  A tile is swept against groups of SW = 64 NA vectors: per step of
//                            32 columns the 64 rows and the SW vectors are decoded into LDS as f32 (decode_chunk, chunk.h:
//                            exact for the three dtypes) and walked with v_mfma_f32_32x32x2_f32.  Wave w owns the row
//                            half w >> 1 and NA 32 x 32 accumulators, vector tiles (w & 1) NA .. (w & 1) NA + NA - 1: one
//                            A operand read from LDS feeds NA MFMAs, and the staged row panel serves SW vectors.
//                            That MFMA is bit for bit a k-ordered fmaf chain (diverse.h), so A[r][j] is ONE chain over
//                            columns 0 .. ld - 1 in order: it depends on the row's and the vector's stored values and d
//                            only -- not on c, j, the range, the tile or NA.  Padding columns are zero in both images,
//                            columns past the row stride are zero in LDS: fma(0, 0, acc) == acc.  fp8: the chain sums
//                            the e4m3 values and the epilogue multiplies once by (scale_r * scale_j).
//                            Arg-max: a lane holds one vector column of 16 rows.  Per row the 64-bit key
//                            score_key << 32 | (0xffffffff - j) (keys.h: unique per j, a tie in key space goes to the
//                            LOWER j, NaN largest) is maximised over the lane's NA accumulators, then over the 32 lanes
//                            of its half wave (xor butterfly), then over the sweeps in registers, and at the end of the
//                            tile over the two waves of a row half with an integer LDS max.
//                            Ragged edges: rows past the range and positions >= c are clamped for addressing, computed,
//                            and never stored or counted (their key is 0, below every real key); a row number is
//                            clamped into [0, n) before it addresses anything.  No load depends on loaded data except
//                            vec_labels[best] and the counts slot, and best < c by construction (and clamped).
//                            Counts: one LDS table of c u32 per workgroup over all its tiles -- live rows only, by the
//                            dead-row bitmap -- merged into HBM with integer atomicAdd.  No float atomics, nothing waits
//                            on another workgroup, plain vector stores.
//                            Floors: HBM, the range's rows read once per sweep (the sweeps after the first out of the
//                            Infinity Cache where the tiles in flight fit); compute, 2 nrows ld max(c, SW) FLOP at the
//                            f32 MFMA rate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk.h"
#include "dead_bits.h"
#include "keys.h"

namespace svs {

constexpr int AS_ROWS = 64;           // corpus rows per tile
constexpr int AS_KT = 32;             // columns per LDS step
constexpr int AS_LDK = AS_KT + 1;     // LDS row stride in floats (odd: the 32 rows a wave half reads fall into 32 banks)
constexpr int AS_THREADS = 256;
constexpr int AS_MAX_VECTORS = 1024;
constexpr int AS_GRID_MAX = 2048;     // workgroups of a launch; more tiles -> more tiles each

typedef float as_f32x16 __attribute__((ext_vector_type(16)));

constexpr int assign_sweep(int NA) { return 64 * NA; }   // vectors per sweep

// M: rows of ld16 16-byte chunks (DT: 0 f32, 1 f16, 2 fp8), n of them; V: the c vectors in the same layout.  The range is
// local rows [r0, r0 + nrows), 0 <= r0, r0 + nrows <= n, nrows >= 1, 1 <= c <= AS_MAX_VECTORS.  out_best / out_scores:
// [nrows]; labels: the index's column (local rows) with vec_labels[c]; counts[c], zero on entry.  Each of the four may be
// null.  dead_bits: null when no row is tombstoned.
template <int DT, int NA>
__global__ __launch_bounds__(AS_THREADS) void assign_rows_kernel(
    const u32x4* __restrict__ M, int ld16, const float* __restrict__ row_scales, int64_t n, const u32x4* __restrict__ V,
    const float* __restrict__ vec_scales, int c, int64_t r0, int64_t nrows, const uint32_t* __restrict__ dead_bits,
    const uint32_t* __restrict__ vec_labels, int32_t* __restrict__ out_best, float* __restrict__ out_scores,
    uint32_t* __restrict__ labels, unsigned long long* __restrict__ counts) {
  constexpr int EPC = elems_per_chunk(DT);
  constexpr int EB = 16 / EPC;                           // 16-byte chunks per 16 elements
  constexpr int SW = assign_sweep(NA);
  constexpr int UNITS = 2 * (AS_ROWS + SW);              // (panel row, half of the step's 32 columns)
  constexpr int NU = (UNITS + AS_THREADS - 1) / AS_THREADS;
  __shared__ float P[AS_ROWS + SW][AS_LDK];              // the corpus rows, then the sweep's vectors: [row][column of the step]
  __shared__ float S[AS_ROWS + SW];                      // fp8: their scales
  __shared__ unsigned long long s_best[AS_ROWS];
  __shared__ uint32_t s_cnt[AS_MAX_VECTORS];
  for (int i = threadIdx.x; i < c; i += AS_THREADS) s_cnt[i] = 0u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave >> 1, wv = (wave & 1) * NA, half = lane >> 5;
  const float* pa = &P[wi * 32 + (lane & 31)][half];
  const float* pb = &P[AS_ROWS + wv * 32 + (lane & 31)][half];   // accumulator a: + a * 32 rows
  const int ksteps = (ld16 * EPC + AS_KT - 1) / AS_KT;   // the whole row stride: the padding columns are zero
  const int64_t ntiles = (nrows + AS_ROWS - 1) / AS_ROWS;
  const u32x4* src[NU];
  u32x4 buf[NU][EB];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (the trip count is the workgroup's)
    const int64_t t0 = tile * AS_ROWS;                   // first row of the tile, relative to r0
    if (threadIdx.x < AS_ROWS) s_best[threadIdx.x] = 0ull;
    unsigned long long best[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) best[r] = 0ull;
    for (int v0 = 0; v0 < c; v0 += SW) {
      // ---- loader: unit u = thread + 256 i holds 16 columns (half u & 1) of panel row u >> 1
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = threadIdx.x + i * AS_THREADS;
        const int pr = u >> 1;
        if (u < 2 * AS_ROWS) {
          int64_t row = r0 + t0 + pr;
          row = row < 0 ? 0 : (row < n ? row : n - 1);
          src[i] = M + row * ld16;
          if (DT == 2 && (u & 1) == 0) S[pr] = row_scales[row];
        } else {
          int pos = v0 + (pr - AS_ROWS);
          pos = pos < c ? pos : c - 1;
          src[i] = V + (int64_t)pos * ld16;
          if (DT == 2 && (u & 1) == 0 && u < UNITS) S[pr] = vec_scales[pos];
        }
      }
      auto fetch = [&](int ks) {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int u = threadIdx.x + i * AS_THREADS;
          const int ch0 = (ks * AS_KT + (u & 1) * 16) / EPC;
#pragma unroll
          for (int e = 0; e < EB; ++e) buf[i][e] = (u < UNITS && ch0 + e < ld16) ? src[i][ch0 + e] : (u32x4){0u, 0u, 0u, 0u};
        }
      };
      auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < NU; ++i) {
          const int u = threadIdx.x + i * AS_THREADS;
          if (u < UNITS) {
            float* o = &P[u >> 1][(u & 1) * 16];
#pragma unroll
            for (int e = 0; e < EB; ++e) {
              float v[EPC];
              decode_chunk<DT>(buf[i][e], v);
#pragma unroll
              for (int j = 0; j < EPC; ++j) o[e * EPC + j] = v[j];
            }
          }
        }
      };
      // ---- MFMA: lane l feeds A[i = l & 31][k = l >> 5], B[k][j = l & 31]
      as_f32x16 acc[NA];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
      fetch(0);
      for (int ks = 0; ks < ksteps; ++ks) {
        stash();
        __syncthreads();
        if (ks + 1 < ksteps) fetch(ks + 1);   // in flight under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < AS_KT; kk += 2) {
          const float av = pa[kk];
#pragma unroll
          for (int a = 0; a < NA; ++a) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pb[a * 32 * AS_LDK + kk], acc[a], 0, 0, 0);
        }
        __syncthreads();
      }
      // ---- epilogue: C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int li = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        unsigned long long key = 0ull;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
          const int lj = (wv + a) * 32 + (lane & 31);
          const uint32_t gj = (uint32_t)(v0 + lj);
          float v = acc[a][r];
          if constexpr (DT == 2) v = v * (S[li] * S[AS_ROWS + lj]);
          const unsigned long long k = gj < (uint32_t)c ? ((unsigned long long)score_key(v) << 32) | (0xffffffffu - gj) : 0ull;
          key = k > key ? k : key;
        }
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {   // over the 32 lanes of the half wave: they hold the row's other columns
          const unsigned long long o = __shfl_xor(key, off, 64);
          key = o > key ? o : key;
        }
        best[r] = key > best[r] ? key : best[r];
      }
      if constexpr (DT == 2) __syncthreads();   // the scales are read above and rewritten by the next sweep
    }
    // ---- the two waves of a row half meet in LDS (zeroed before the first step's barrier)
    if ((lane & 31) == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) atomicMax(&s_best[wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half], best[r]);
    }
    __syncthreads();
    if (threadIdx.x < AS_ROWS && t0 + threadIdx.x < nrows) {
      const int64_t i = t0 + threadIdx.x, row = r0 + i;
      const unsigned long long key = s_best[threadIdx.x];
      uint32_t j = 0xffffffffu - (uint32_t)key;
      j = j < (uint32_t)c ? j : (uint32_t)c - 1u;   // (always: position 0 is real, so the key is one)
      if (out_best) out_best[i] = (int32_t)j;
      if (out_scores) out_scores[i] = key_score((uint32_t)(key >> 32));
      if (labels) labels[row] = vec_labels[j];
      if (counts) {
        if (!row_dead(dead_bits, row)) atomicAdd(&s_cnt[j], 1u);
      }
    }
    __syncthreads();   // s_best before the next tile zeroes it; s_cnt before the merge
  }
  if (counts)
    for (int i = threadIdx.x; i < c; i += AS_THREADS) {
      const uint32_t k = s_cnt[i];
      if (k) atomicAdd(&counts[i], (unsigned long long)k);
    }
}

}  // namespace svs

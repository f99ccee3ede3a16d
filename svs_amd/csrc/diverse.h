// Diverse retrieval (svs_index_search_diverse): maximal-marginal-relevance re-ranking of a search's candidates.
//
// Behind the unchanged top-fetch_k search, per block of queries, two launches on the context's stream:
//
//   diverse_gram_kernel<DT>  G[q][i][j] = <stored row of candidate i, stored row of candidate j>, c x c per query.
//                            Grid: the upper-triangle 64 x 64 tiles (tile_i <= tile_j) x the block's queries; a tile off the
//                            diagonal also stores its mirror image.  A workgroup gathers its two panels of 64 rows through
//                            the query's candidate list (global rows, 64-bit addressing row * ld16 as gather.h), decodes
//                            32 columns of each into LDS as f32 (decode_chunk, chunk.h: f32 as is, f16 widened, fp8 e4m3
//                            -> f32, all exact) and
//                            walks them with v_mfma_f32_32x32x2_f32, one 32 x 32 accumulator per wave.  That MFMA is bit for
//                            bit a k-ordered fmaf chain, so G[i][j] is ONE chain over columns 0 .. ld-1 in order: it depends
//                            on the two rows' stored values and d only -- not on the tile, the position, c or nq -- and
//                            a * b == b * a makes it symmetric bit for bit.  The padding columns are zero in HBM, columns past
//                            the row stride are zero in LDS: fma(0, 0, acc) == acc.  fp8: the chain sums the e4m3 values and
//                            the epilogue multiplies by (scale_i * scale_j), a commutative product.
//                            Ragged edges: list positions >= c are clamped to c - 1 (computed, never stored); a row number
//                            is clamped into [0, n) before it addresses anything.
//                            Roofline: compute, 2 c^2 d FLOP at the f32 MFMA rate (half of it with the mirror); the rows
//                            (c x row bytes, 6 MB at c = 1024 x 1536 f32) are re-read c / 64 times out of L2.
//
//   diverse_pick_kernel      one workgroup per query: scores, redundancy and the picked flags of the c candidates in LDS.
//                            count - 1 steps; a step reads row `last pick` of G (4 KiB, L2), red = max(red, G), obj =
//                            lambda * s - (1 - lambda) * red, and a block arg-max over (obj desc, position asc) among the
//                            unpicked.  A NaN objective ranks as -inf, so every step picks an unpicked position whatever
//                            the data holds; the loop is bounded by count.  No atomics, nothing waits on another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk.h"

namespace svs {

constexpr int DV_TILE = 64;        // candidates per tile side
constexpr int DV_KT = 32;          // columns per LDS step
constexpr int DV_LDK = DV_KT + 1;  // LDS row stride in floats (odd: the 32 rows a wave half reads fall into 32 banks)
constexpr int DV_THREADS = 256;
constexpr int DV_PICK_THREADS = 256;
constexpr int DV_MAX_FETCH = 1024;
constexpr int DV_PPT = DV_MAX_FETCH / DV_PICK_THREADS;   // positions per thread of the pick kernel

typedef float dv_f32x16 __attribute__((ext_vector_type(16)));

// tiles per side nt; linear index x over the pairs (ti <= tj), row-major
__device__ __forceinline__ void dv_tile_of(int x, int nt, int* ti, int* tj) {
  int i = 0;
  while (x >= nt - i) {
    x -= nt - i;
    ++i;
  }
  *ti = i;
  *tj = i + x;
}

// M: rows of ld16 16-byte chunks (DT: 0 f32, 1 f16, 2 fp8); cand: [queries][c] global rows (a search's output);
// G: [queries][c][c].  Grid: (nt (nt + 1) / 2, queries).
template <int DT>
__global__ __launch_bounds__(DV_THREADS) void diverse_gram_kernel(
    const u32x4* __restrict__ M, int ld16, const float* __restrict__ row_scales, const int64_t* __restrict__ cand, int c,
    int64_t row_offset, int64_t n, int nt, float* __restrict__ G) {
  constexpr int EPC = elems_per_chunk(DT);
  constexpr int EB = 16 / EPC;                          // bytes per element = 16-byte chunks per 16 elements
  __shared__ float P[2][DV_TILE][DV_LDK];               // the two panels, [row][column of the step]
  __shared__ float S[2][DV_TILE];                       // fp8: the rows' scales
  int ti, tj;
  dv_tile_of((int)blockIdx.x, nt, &ti, &tj);
  cand += (int64_t)blockIdx.y * c;
  G += (int64_t)blockIdx.y * c * c;
  // ---- loader: thread t holds 16 columns (half h) of row rr of panel pn
  const int pn = threadIdx.x >> 7, rr = (threadIdx.x >> 1) & (DV_TILE - 1), h = threadIdx.x & 1;
  int pos = (pn ? tj : ti) * DV_TILE + rr;
  pos = pos < c ? pos : c - 1;
  int64_t row = cand[pos] - row_offset;
  row = row < 0 ? 0 : (row < n ? row : n - 1);
  const u32x4* src = M + row * ld16;
  if (DT == 2 && h == 0) S[pn][rr] = row_scales[row];
  const int ksteps = (ld16 * EPC + DV_KT - 1) / DV_KT;   // the whole row stride: the padding columns are zero
  u32x4 buf[EB];
  auto fetch = [&](int ks) {
    const int ch0 = (ks * DV_KT + h * 16) / EPC;
#pragma unroll
    for (int e = 0; e < EB; ++e) buf[e] = ch0 + e < ld16 ? src[ch0 + e] : (u32x4){0u, 0u, 0u, 0u};
  };
  auto stash = [&]() {
    float* o = &P[pn][rr][h * 16];
#pragma unroll
    for (int e = 0; e < EB; ++e) {
      float v[EPC];
      decode_chunk<DT>(buf[e], v);
#pragma unroll
      for (int j = 0; j < EPC; ++j) o[e * EPC + j] = v[j];
    }
  };
  // ---- MFMA: wave w owns the 32 x 32 block (wi, wj) of the tile; lane l feeds A[i = l & 31][k = l >> 5], B[k][j = l & 31]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = wave >> 1, wj = wave & 1;
  const float* pa = &P[0][wi * 32 + (lane & 31)][lane >> 5];
  const float* pb = &P[1][wj * 32 + (lane & 31)][lane >> 5];
  dv_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  fetch(0);
  for (int ks = 0; ks < ksteps; ++ks) {
    stash();
    __syncthreads();
    if (ks + 1 < ksteps) fetch(ks + 1);   // in flight under this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < DV_KT; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
    __syncthreads();
  }
  // ---- epilogue: C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int lj = wj * 32 + (lane & 31);
  const int gj = tj * DV_TILE + lj;
  const float sj = DT == 2 ? S[1][lj] : 1.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int li = wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    const int gi = ti * DV_TILE + li;
    if (gi < c && gj < c) {
      float v = acc[r];
      if constexpr (DT == 2) v = v * (S[0][li] * sj);
      G[(int64_t)gi * c + gj] = v;
      if (ti != tj) G[(int64_t)gj * c + gi] = v;
    }
  }
}

// (obj desc, position asc); obj is never NaN here
__device__ __forceinline__ bool dv_better(float ao, int ap, float bo, int bp) { return ao > bo || (ao == bo && ap < bp); }

// cand_s / cand_r: [queries][c] (the search's output, score desc / row desc); G: [queries][c][c]; out_*: [queries][count].
// 2 <= count <= c <= DV_MAX_FETCH.  Grid: one workgroup per query.
__global__ __launch_bounds__(DV_PICK_THREADS) void diverse_pick_kernel(
    const float* __restrict__ cand_s, const int64_t* __restrict__ cand_r, const float* __restrict__ G, int c, int count,
    float lam, float oml, float* __restrict__ out_s, int64_t* __restrict__ out_r, float* __restrict__ out_red) {
  __shared__ float s[DV_MAX_FETCH], red[DV_MAX_FETCH];
  __shared__ uint8_t picked[DV_MAX_FETCH];
  __shared__ float w_obj[DV_PICK_THREADS / 64];
  __shared__ int w_pos[DV_PICK_THREADS / 64];
  const int q = blockIdx.x;
  cand_s += (int64_t)q * c;
  cand_r += (int64_t)q * c;
  G += (int64_t)q * c * c;
  out_s += (int64_t)q * count;
  out_r += (int64_t)q * count;
  if (out_red) out_red += (int64_t)q * count;
  const float NEG_INF = -__builtin_inff();
  for (int p = threadIdx.x; p < c; p += DV_PICK_THREADS) {
    s[p] = cand_s[p];
    red[p] = NEG_INF;
    picked[p] = p == 0;
  }
  if (threadIdx.x == 0) {
    out_s[0] = cand_s[0];
    out_r[0] = cand_r[0];
    if (out_red) out_red[0] = NEG_INF;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int last = 0;
  for (int t = 1; t < count; ++t) {
    const float* g = G + (int64_t)last * c;
    float bo = NEG_INF;
    int bp = 0x7fffffff;   // (no unpicked position seen)
#pragma unroll
    for (int u = 0; u < DV_PPT; ++u) {
      const int p = threadIdx.x + u * DV_PICK_THREADS;   // ascending per thread: the first best is the lowest
      if (p < c && !picked[p]) {
        const float r = fmaxf(red[p], g[p]);
        red[p] = r;
        float o = lam * s[p] - oml * r;
        o = o == o ? o : NEG_INF;
        if (dv_better(o, p, bo, bp)) { bo = o; bp = p; }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float oo = __shfl_xor(bo, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (dv_better(oo, op, bo, bp)) { bo = oo; bp = op; }
    }
    if (lane == 0) { w_obj[wave] = bo; w_pos[wave] = bp; }
    __syncthreads();
    bo = w_obj[0];
    bp = w_pos[0];
#pragma unroll
    for (int w = 1; w < DV_PICK_THREADS / 64; ++w)
      if (dv_better(w_obj[w], w_pos[w], bo, bp)) { bo = w_obj[w]; bp = w_pos[w]; }
    // (count <= c: an unpicked position exists, and -inf at a real position beats the empty mark)
    last = bp < c ? bp : 0;
    if (threadIdx.x == 0) {
      picked[last] = 1;
      out_s[t] = s[last];
      out_r[t] = cand_r[last];
      if (out_red) out_red[t] = red[last];
    }
    __syncthreads();   // the flag and w_* before the next step
  }
}

}  // namespace svs

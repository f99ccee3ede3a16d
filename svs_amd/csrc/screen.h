// Screened single-query search over an f32 corpus ("Screened search").
//
// An f32 index keeps an IEEE-half SHADOW of its rows in HBM.  One query then costs
//   1. the f16 one-shot kernel (gemv_f16.h) over the shadow: approximate scores a_r, half the bytes;
//   2. the window histogram of select.h over a;
//   3. screen_filter_kernel: every row that can still be in the exact top-k, from a proven bound
//      E >= |a_r - s_r| (s_r the f32 kernel's score): the rows with a_r >= v* - 2E, v* <= the k-th best a;
//   4. rescore_f32_kernel: the exact score of those rows from the f32 corpus, with row_dot_f32 -- the
//      arithmetic of gemv_f32.h's kernels, so the bits are theirs;
//   5. select_final_kernel ranks them.
// Whenever the bound cannot be applied (k-th best not positive, non-finite query, more than CAND_CAP rows
// inside the margin) step 4 scores the WHOLE f32 corpus instead and step 5 takes its exact path over the
// raw scores: always the unscreened answer, never an approximation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"
#include "gemv_f16.h"
#include "gemv_f32.h"
#include "keys.h"
#include "select.h"

namespace svs {

// Per-corpus statistics of the shadow, reduced by shadow_rows_kernel: float bits of non-negative values
// (so unsigned max is float max), each rounded up.  Monotone: appended rows only raise them.
//   A = max_r ||m_r - half(m_r)||   B = max_r ||half(m_r)||   C = max_r ||m_r||
//   bad != 0: some element is not finite or overflows half (|x| > 65504): the index never screens.
struct ScreenStats {
  uint32_t A, B, C, bad;
};

// Per search context, in device memory and mirrored to pinned host memory by the kernels (plain stores):
//   [0] screened queries  [1] queries that took the exact fallback  [2] bits of the last E  [3] last n_cand
constexpr int SCREEN_SLOT_WORDS = 4;

constexpr float SCREEN_UP = 1.001f;   // a norm from an f32 sum of <= 4096 squares is within 2.5e-4 of the truth
constexpr float SCREEN_C = 1.01f;     // f32 evaluation of E itself

__device__ __forceinline__ float wave_sum_xor(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// f32 rows [row0, row0 + nrows) AS STORED (stride ld4 float4) -> half rows of the same stride in elements,
// and the statistics above.  One wave per row, grid-stride.
__global__ __launch_bounds__(256) void shadow_rows_kernel(const v4f* __restrict__ rows, int64_t row0, int64_t nrows,
                                                          int ld4, uint2* __restrict__ shadow,
                                                          ScreenStats* __restrict__ st) {
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t W = (int64_t)gridDim.x * 4;
  float mA = 0.f, mB = 0.f, mC = 0.f;
  bool bad = false;
  for (int64_t r = gw; r < nrows; r += W) {
    const v4f* p = rows + (row0 + r) * ld4;
    uint2* o = shadow + (row0 + r) * ld4;
    float e2 = 0.f, b2 = 0.f, c2 = 0.f;
    for (int c = lane; c < ld4; c += 64) {
      const v4f x = __builtin_nontemporal_load(p + c);
      const h2 lo = {(_Float16)x.x, (_Float16)x.y}, hi = {(_Float16)x.z, (_Float16)x.w};
      o[c] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
      const float xs[4] = {x.x, x.y, x.z, x.w};
      const float hs[4] = {(float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dl = xs[e] - hs[e];
        e2 = fmaf(dl, dl, e2);
        b2 = fmaf(hs[e], hs[e], b2);
        c2 = fmaf(xs[e], xs[e], c2);
        bad = bad || !(fabsf(xs[e]) <= 65504.f);   // (also true for NaN)
      }
    }
    mA = fmaxf(mA, wave_sum_xor(e2));
    mB = fmaxf(mB, wave_sum_xor(b2));
    mC = fmaxf(mC, wave_sum_xor(c2));
  }
  const bool any_bad = __any(bad);
  if (lane == 0) {
    if (any_bad) atomicOr(&st->bad, 1u);
    // (a NaN sum only happens with `bad`; non-negative floats order like their bits)
    if (mA > 0.f) atomicMax(&st->A, f32_bits(sqrtf(mA) * SCREEN_UP));
    if (mB > 0.f) atomicMax(&st->B, f32_bits(sqrtf(mB) * SCREEN_UP));
    if (mC > 0.f) atomicMax(&st->C, f32_bits(sqrtf(mC) * SCREEN_UP));
  }
}

// The bound E >= |a_r - s_r| for every row r of the corpus (derivation: DESIGN.md), from the three query
// norms nq = ||q||, nh = ||half(q)||, ne = ||q - half(q)|| (each rounded up) and the corpus statistics.
// t = ld + 16 roundings, u = 2^-24.  Any NaN / inf input gives a NaN / inf E, which the caller treats as
// "no bound".
__device__ __forceinline__ float screen_bound(float nq, float nh, float ne, float A, float B, float C, int ld) {
  const float tu = (float)(ld + 16) * 5.9604645e-8f;
  const float gamma = tu / (1.f - tu);
  const float tiny = 1e-30f + 1e-17f * (nq + B);   // squares and products that underflow
  return SCREEN_C * (ne * B + nq * A + gamma * (nh * B + nq * C)) + tiny;
}

// ---- step 3.  grid = blocks (one query); q: the query as the score kernels read it (ld floats) ----
__global__ __launch_bounds__(FA_THREADS) void screen_filter_kernel(
    const float* __restrict__ scores, int64_t n, uint32_t k, uint32_t* __restrict__ scratch,
    uint64_t* __restrict__ cand, const float* __restrict__ q, int ld, const ScreenStats* __restrict__ stats,
    uint32_t* __restrict__ slot_host) {
  __shared__ uint32_t sh[FA_THREADS + 2];
  __shared__ float red[3][FA_THREADS / 64];
  const sel_v4f* s4 = (const sel_v4f*)scores;
  SelHeader* hdr = (SelHeader*)scratch;
  const uint32_t* hist = scratch + sizeof(SelHeader) / 4;
  const int64_t n4 = (n + 3) >> 2;
  const int64_t base = ((int64_t)blockIdx.x * SEL_VPT) * FA_THREADS + threadIdx.x;
  sel_v4f v[SEL_VPT];
#pragma unroll
  for (int j = 0; j < SEL_VPT; ++j) {
    const int64_t i4 = base + (int64_t)j * FA_THREADS;
    v[j] = i4 < n4 ? s4[i4] : (sel_v4f){0.f, 0.f, 0.f, 0.f};
  }
  // the query's norms (every workgroup sums the same values in the same order: one E for the whole grid)
  float x2 = 0.f, h2s = 0.f, e2 = 0.f;
  for (int i = threadIdx.x; i < ld; i += FA_THREADS) {
    const float x = q[i];
    const float h = (float)(_Float16)x;
    const float dl = x - h;
    x2 = fmaf(x, x, x2);
    h2s = fmaf(h, h, h2s);
    e2 = fmaf(dl, dl, e2);
  }
  x2 = wave_sum_xor(x2);
  h2s = wave_sum_xor(h2s);
  e2 = wave_sum_xor(e2);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = x2;
    red[1][threadIdx.x >> 6] = h2s;
    red[2][threadIdx.x >> 6] = e2;
  }
  uint32_t bstar, krank;
  pick_bucket<FA_THREADS>(hist, WBINS, k, sh, &bstar, &krank);   // (its barriers publish red[])
  float sx = 0.f, sh2 = 0.f, se = 0.f;
#pragma unroll
  for (int w = 0; w < FA_THREADS / 64; ++w) {
    sx += red[0][w];
    sh2 += red[1][w];
    se += red[2][w];
  }
  const float E = screen_bound(sqrtf(sx) * SCREEN_UP, sqrtf(sh2) * SCREEN_UP, sqrtf(se) * SCREEN_UP,
                               bits_f32(stats->A), bits_f32(stats->B), bits_f32(stats->C), ld);
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (first && slot_host) slot_host[2] = f32_bits(E);
  // v* = lower edge of the bin of the k-th best approximate score (<= that score); cut = v* - 2E must be a
  // finite value inside the window, PROVABLY: every comparison is written so that NaN / inf fail it.
  bool ok = bstar != 0xffffffffu;
  float cut = 0.f;
  if (ok) {
    const float vstar = key_score((WBASE + bstar) << 16);
    cut = vstar - 2.f * E;
    ok = cut >= key_score(WBASE << 16) && cut <= vstar;
  }
  if (!ok) {   // the re-score kernel then scores the whole corpus exactly
    if (first) hdr->flag = 1;
    return;
  }
  filter_compact(v, base, n, window_bin(score_key(cut)), hdr, cand);
}

// ---- step 4.  Persistent grid of 4-wave workgroups; ld == NSTEP * 256 floats ----
// Normal case: wave w takes candidates w*U .. w*U + U-1, then strides by the grid: U whole rows in flight
// (NSTEP wave-wide 16-byte loads each, all requested before the first FMA), and replaces each entry's key
// by the key of the exact score.  Fallback (flag set by the filter, or the list overflowed): the same
// grid scores ALL rows into `scores` (tombstoned rows -> -inf), for select_final_kernel's exact path.
// cnt_dev / slot_host: this context's counters (device copy, pinned mirror).
template <int NSTEP, int U>
__global__ __launch_bounds__(256) void rescore_f32_kernel(
    const v4f* __restrict__ M, const v4f* __restrict__ q, float* __restrict__ scores, int64_t n,
    const uint32_t* __restrict__ scratch, uint64_t* __restrict__ cand, const uint32_t* __restrict__ dead_bits,
    uint32_t* __restrict__ cnt_dev, uint32_t* __restrict__ slot_host) {
  constexpr int LD4 = NSTEP * 64;
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t W = (int64_t)gridDim.x * 4;
  const SelHeader* hdr = (const SelHeader*)scratch;
  const uint32_t flag = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr->flag);
  const uint32_t n_cand = (uint32_t)__builtin_amdgcn_readfirstlane((int)hdr->n_cand);
  const bool fallback = flag != 0u || n_cand > (uint32_t)CAND_CAP;
  if (gw == 0 && lane == 0) {   // (searches on one context are stream-ordered: no other writer)
    const uint32_t c = cnt_dev[fallback ? 1 : 0] + 1u;
    cnt_dev[fallback ? 1 : 0] = c;
    slot_host[fallback ? 1 : 0] = c;
    slot_host[3] = n_cand;
  }
  v4f qv[NSTEP];
#pragma unroll
  for (int j = 0; j < NSTEP; ++j) qv[j] = q[j * 64 + lane];
  v4f buf[U][NSTEP];
  if (!fallback) {
    for (int64_t i = gw * U; i < (int64_t)n_cand; i += W * U) {
      uint32_t row[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = i + u < (int64_t)n_cand ? i + u : (int64_t)n_cand - 1;
        row[u] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)cand[p]);   // (the row half of an entry never changes)
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const v4f* p = M + (int64_t)row[u] * LD4 + lane;
#pragma unroll
        for (int j = 0; j < NSTEP; ++j) buf[u][j] = ldg4<true>(p + j * 64);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float s = row_dot_f32<NSTEP>(buf[u], qv);
        if (lane == 0 && i + u < (int64_t)n_cand) cand[i + u] = make_key(s, row[u]);
      }
    }
  } else {
    for (int64_t r = gw * U; r < n; r += W * U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t row = r + u < n ? r + u : n - 1;
        const v4f* p = M + row * LD4 + lane;
#pragma unroll
        for (int j = 0; j < NSTEP; ++j) buf[u][j] = ldg4<true>(p + j * 64);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float s = row_dot_f32<NSTEP>(buf[u], qv);
        const int64_t row = r + u;
        if (lane == 0 && row < n) {
          if (row_dead(dead_bits, row)) s = -__builtin_inff();
          scores[row] = s;
        }
      }
    }
  }
}

}  // namespace svs

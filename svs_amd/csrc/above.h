// Threshold search (svs_index_search_above): every live row whose score is at or above a caller-given cut-off,
// best first, and how many there are.
//
// The cut is made in KEY space (keys.h), the space the order is defined in: row r qualifies iff
// score_key(s[r]) >= score_key(cut-off).  So -0.0 and +0.0 are one cut-off, a NaN score qualifies for every
// cut-off and sorts first (as in the top-k searches), and -inf admits every live row.  Tombstoned rows are left out
// by the dead-row BITMAP, never by their score: a masked score of -inf would pass a cut-off of -inf.
//
// Two launches behind the unchanged single-query score pass, on the context's stream:
//   1. above_filter_kernel: the grid of select_window_filter_kernel over the score vector; the survivors are
//      appended as (key << 32 | row) to the context's candidate list (wave-aggregated, as filter_compact), and
//      SelHeader::n_cand counts ALL of them, also those past CAND_CAP: the total is exact when the list is not.
//   2. above_final_kernel, one workgroup: writes the total; while the list is whole (total <= CAND_CAP) and the
//      wanted prefix fits the LDS sort (min(limit, total) <= SORT_CAP) it orders the list and emits the prefix --
//      the device-complete zone.  Otherwise it writes count = -1 and the host re-runs that query through the exact
//      top-k stage with k = min(limit, total): the best that many live rows ARE the first that many of the answer.
// The output length is decided on the device; the host waits once per call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"
#include "keys.h"
#include "select.h"

namespace svs {

// grid = blocks of FA_THREADS * SEL_VPT float4 groups over scores[0 .. n); tkey = score_key(cut-off);
// dead_bits: the dead-row bitmap (dead_bits.h), null when no row is masked; hdr / cand: one query's
// SelHeader (zero on entry) and candidate list of CAND_CAP entries.
__global__ __launch_bounds__(FA_THREADS) void above_filter_kernel(
    const float* __restrict__ scores, int64_t n, uint32_t tkey, const uint32_t* __restrict__ dead_bits,
    uint32_t* __restrict__ scratch, uint64_t* __restrict__ cand) {
  SelHeader* hdr = (SelHeader*)scratch;
  const sel_v4f* s4 = (const sel_v4f*)scores;
  const int64_t n4 = (n + 3) >> 2;   // the allocation is padded to a multiple of 4
  const int64_t base = ((int64_t)blockIdx.x * SEL_VPT) * FA_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  sel_v4f v[SEL_VPT];
  uint32_t dead[SEL_VPT];
#pragma unroll
  for (int j = 0; j < SEL_VPT; ++j) {   // all requested before the first is used
    const int64_t i4 = base + (int64_t)j * FA_THREADS;
    v[j] = i4 < n4 ? s4[i4] : (sel_v4f){0.f, 0.f, 0.f, 0.f};
    dead[j] = dead_nibble(i4 < n4 ? dead_bits : nullptr, i4);
  }
#pragma unroll
  for (int j = 0; j < SEL_VPT; ++j) {
    const int64_t i = (base + (int64_t)j * FA_THREADS) * 4;
    uint32_t key[4];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      key[e] = 0;
      if (i + e < n && !((dead[j] >> e) & 1u)) {
        const uint32_t kk = score_key(v[j][e]);
        if (kk >= tkey) {
          key[e] = kk;
          ++cnt;
        }
      }
    }
    // wave-aggregated append: one atomic per wave per group that has survivors
    const unsigned long long m = __ballot(cnt > 0);
    if (m) {
      int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
      }
      const int total = __shfl(incl, 63, 64);
      uint32_t wbase = 0;
      if (lane == 0) wbase = atomicAdd(&hdr->n_cand, (uint32_t)total);
      wbase = __shfl(wbase, 0, 64);
      uint32_t slot = wbase + (uint32_t)(incl - cnt);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (key[e]) {   // a real key is never 0 (score_key's minimum is 0x007fffff)
          if (slot < (uint32_t)CAND_CAP) cand[slot] = ((uint64_t)key[e] << 32) | (uint32_t)(i + e);
          ++slot;
        }
      }
    }
  }
}

// One workgroup.  limit: the caller's, clamped to [0, live rows]; out_scores / out_rows hold min(limit, SORT_CAP)
// entries (unused when limit == 0); *out_count = entries written, or -1: the host re-runs the query; *out_total =
// qualifying rows, always.  Leaves the SelHeader zeroed for the next user of the context (select_final_kernel's
// convention; the histogram words behind it were never touched).
__global__ __launch_bounds__(FINAL_THREADS) void above_final_kernel(
    uint32_t* __restrict__ scratch, const uint64_t* __restrict__ cand, int limit, int64_t row_offset,
    float* __restrict__ out_scores, int64_t* __restrict__ out_rows, int32_t* __restrict__ out_count,
    int64_t* __restrict__ out_total) {
  __shared__ __attribute__((aligned(16))) uint64_t S[SORT_CAP];
  __shared__ uint32_t lh[RS_BINS];
  __shared__ uint32_t sh[256 + 2];
  __shared__ uint32_t s_cnt;
  SelHeader* hdr = (SelHeader*)scratch;
  const uint32_t total = hdr->n_cand;
  const int want = (uint32_t)limit < total ? limit : (int)total;   // (limit >= 0)
  const bool complete = want == 0 || (total <= (uint32_t)CAND_CAP && want <= SORT_CAP);
  __syncthreads();   // every thread has read the header
  if (threadIdx.x == 0) {
    hdr->n_cand = 0;
    hdr->flag = 0;
    *out_total = (int64_t)total;
    *out_count = complete ? want : -1;
  }
  if (!complete || want == 0) return;
  int m;
  if (total <= (uint32_t)SORT_CAP) {
    m = next_pow2((int)total < 2 ? 2 : (int)total);
    for (int i = threadIdx.x; i < m; i += blockDim.x) S[i] = i < (int)total ? cand[i] : 0ull;
  } else {
    // the want-th largest key of the list; the keys at or above it (exactly `want`: keys are unique) are sorted
    if (threadIdx.x == 0) s_cnt = 0;
    m = next_pow2(want < 2 ? 2 : want);
    for (int i = threadIdx.x; i < m; i += blockDim.x) S[i] = 0ull;
    auto key_at = [&](int64_t i) { return cand[i]; };
    const uint64_t T = block_radix_select(key_at, (int64_t)total, (uint32_t)want, lh, sh);
    for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) {
      const uint64_t key = cand[i];
      if (key >= T) {
        const uint32_t slot = atomicAdd(&s_cnt, 1u);
        if (slot < (uint32_t)SORT_CAP) S[slot] = key;
      }
    }
  }
  __syncthreads();
  if (m <= FINAL_THREADS) {
    emit_by_rank(S, m, want, want, row_offset, out_scores, out_rows);
  } else {
    bitonic_sort_lds_desc(S, m);
    emit_topk(S, want, want, row_offset, out_scores, out_rows);
  }
}

}  // namespace svs

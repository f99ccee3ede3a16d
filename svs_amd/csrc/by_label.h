// Per-label breakdown (svs_index_search_by_label): for every label of a caller-given set, how many live rows of that
// label score at or above a cut-off and which of them is the best -- facet counts plus one best hit per facet, the
// groups ordered by their best row.
//
// The cut is made in KEY space as in above.h (-0.0 == +0.0, a NaN score qualifies for every cut-off and sorts first,
// -inf admits every live row); tombstoned rows leave through the dead-row BITMAP.  A group's reduction is the MAX of
// the order's own unique 64-bit key (keys.h) plus an INTEGER count: both are independent of arrival order, so the
// answer is exact and bit-reproducible however the workgroups are scheduled.
//
// Two launches behind the unchanged single-query score pass, on the context's stream:
//   1. by_label_reduce_kernel<CROSS>: workgroups stride over strips of BL_STRIP rows.  A thread takes BL_VPT groups of
//      four consecutive rows per strip: a 16-byte load of the four scores, one of their four labels, and one nibble of
//      a bitmap word, every load requested before the first is used.  A qualifying row's label is searched in the
//      set's LDS image (label_stage_set, label_slot): its SLOT is its index in the sorted set.  Each workgroup keeps a private table in LDS -- a u32 count and a u64 best key per
//      slot, 12 KiB at 1,024 labels -- updated with LDS atomics (add, max).  Before that the wave aggregates the slot
//      of its first hit (wave_fold_top): the lanes that share it become ONE add and ONE max (one label holding every row: 2 LDS
//      atomics per wave and element instead of 128 on one address); the other lanes update on their own.
//      What crosses workgroups:
//        BL_ATOMIC    the non-empty slots go to the query's table in HBM with integer atomicAdd (u64) / atomicMax (u64);
//        BL_PARTIALS  every workgroup writes its whole table as one partial; the final kernel reduces the partials --
//                     nothing crosses but through the kernel boundary.
//      Both are sums and maxima of integers: identical bits.  No workgroup waits for another, nothing spins, no
//      float atomics.  The grid is capped at BL_GRID_MAX workgroups, so the partials are bounded at any row count.
//   2. by_label_final_kernel, one workgroup per query: gathers the table (or reduces the partials in LDS), compacts the
//      non-empty slots, ranks their best keys by counting (keys are unique: the number of larger keys IS the
//      position), writes label, score, row and total of the first min(k, |G|) and |G| itself, and leaves the table in
//      HBM zeroed for the next query and the next call (select_final_kernel's convention).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keys.h"
#include "labels.h"
#include "scored_strip.h"

namespace svs {

constexpr int BL_THREADS = 256;
constexpr int BL_VPT = 4;                               // groups of four rows per thread and strip, all loaded before the first is used
constexpr int BL_STRIP = BL_THREADS * BL_VPT * 4;       // rows per strip
constexpr int BL_GRID_MAX = 256;                        // workgroups of the reduce kernel: one per CU; more rows -> more strips each
constexpr int BL_FINAL_THREADS = 1024;
constexpr int BL_ATOMIC = 0, BL_PARTIALS = 1;           // by_label_reduce_kernel's CROSS
constexpr int BL_TAB_WORDS = 2 * LB_MAX_SET;            // the query's table in HBM: best[LB_MAX_SET], then count[LB_MAX_SET], u64 each
static_assert(BL_THREADS == LB_THREADS, "label_stage_set strides by LB_THREADS");
static_assert(BL_STRIP % 32 == 0, "strips begin at whole bitmap words");

// Every lane of the wave calls this (converged): slot < 0 = no hit; key32 = the hit's score key, row = its row.
__device__ __forceinline__ void by_label_update(int slot, uint32_t key32, uint32_t row, unsigned long long* s_best, uint32_t* s_cnt) {
  const unsigned long long hit = __ballot(slot >= 0);
  if (!hit) return;   // (wave-uniform)
  const int lead = __shfl(slot, __ffsll((long long)hit) - 1, 64);
  const bool peer = slot == lead;
  bool top;
  const unsigned long long peers = wave_fold_top(peer, key32, &top);
  if (peers & (peers - 1)) {   // two lanes or more on the leader's slot: one add, one max
    if (top) {
      atomicAdd(&s_cnt[lead], (uint32_t)__popcll(peers));
      atomicMax(&s_best[lead], ((unsigned long long)key32 << 32) | row);
    }
    if (peer) slot = -1;
  }
  if (slot >= 0) {
    atomicAdd(&s_cnt[slot], 1u);
    atomicMax(&s_best[slot], ((unsigned long long)key32 << 32) | row);
  }
}

// grid = min(strips, BL_GRID_MAX) workgroups; f: the label filter (nset >= 1) over scores[0 .. f.n); tkey =
// score_key(cut-off).  BL_ATOMIC: tab = the query's table (BL_TAB_WORDS, zero on entry).  BL_PARTIALS: workgroup g writes
// part_best / part_cnt [g * f.nset .. (g + 1) * f.nset), empty slots included.
template <int CROSS>
__global__ __launch_bounds__(BL_THREADS) void by_label_reduce_kernel(LabelFilter f, const float* __restrict__ scores, uint32_t tkey,
                                                                     unsigned long long* __restrict__ tab,
                                                                     unsigned long long* __restrict__ part_best,
                                                                     uint32_t* __restrict__ part_cnt) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ unsigned long long s_best[LB_MAX_SET];
  __shared__ uint32_t s_cnt[LB_MAX_SET];
  for (int i = threadIdx.x; i < f.nset; i += BL_THREADS) {
    s_best[i] = 0ull;
    s_cnt[i] = 0u;
  }
  label_stage_set(f, s_set);
  __syncthreads();
  // (The strip's loads are spelled out here, not taken from scored_strip.h's ScoredStrip as collapse.h's are: with it
  //  the kernel came out one VGPR larger and, with every row qualifying on f16, 0.5 % slower per call over six runs.)
  const float4* s4 = (const float4*)scores;
  const uint4* l4 = (const uint4*)f.labels;
  const int64_t n4 = (f.n + 3) >> 2;   // both allocations are padded to a multiple of 4
  const int64_t strips = (f.n + BL_STRIP - 1) / BL_STRIP;
  for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {   // (the trip count is the workgroup's: waves stay converged)
    const int64_t base = strip * (BL_STRIP / 4) + threadIdx.x;
    float4 v[BL_VPT];
    uint4 lab[BL_VPT];
    uint32_t dead[BL_VPT];
#pragma unroll
    for (int j = 0; j < BL_VPT; ++j) {   // all requested before the first is used
      const int64_t i4 = base + (int64_t)j * BL_THREADS;
      const bool in = i4 < n4;
      v[j] = in ? s4[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
      lab[j] = (l4 && in) ? l4[i4] : make_uint4(0u, 0u, 0u, 0u);
      dead[j] = dead_nibble(in ? f.dead_bits : nullptr, i4);
    }
#pragma unroll
    for (int j = 0; j < BL_VPT; ++j) {
      const int64_t i = (base + (int64_t)j * BL_THREADS) * 4;
      const float sc[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      const uint32_t lb[4] = {lab[j].x, lab[j].y, lab[j].z, lab[j].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int slot = -1;
        const uint32_t kk = score_key(sc[e]);
        if (i + e < f.n && !((dead[j] >> e) & 1u) && kk >= tkey) slot = label_slot(lb[e], f, s_set);
        by_label_update(slot, kk, (uint32_t)(i + e), s_best, s_cnt);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < f.nset; i += BL_THREADS) {
    const uint32_t c = s_cnt[i];
    if (CROSS == BL_ATOMIC) {
      if (c) {
        atomicAdd(&tab[LB_MAX_SET + i], (unsigned long long)c);
        atomicMax(&tab[i], s_best[i]);
      }
    } else {
      part_best[(int64_t)blockIdx.x * f.nset + i] = s_best[i];
      part_cnt[(int64_t)blockIdx.x * f.nset + i] = c;
    }
  }
}

// One workgroup.  nparts == 0: the table `tab` holds the query's groups and is left zeroed; nparts > 0: the partials of
// nparts workgroups are reduced here.  set[0 .. nset) on the device when nset >= 2, `single` when nset == 1.  k: the
// caller's; the four result arrays hold min(max(k, 0), nset) entries (unused when that is 0).  *out_count = entries
// written, *out_groups = the labels with a qualifying row.
__global__ __launch_bounds__(BL_FINAL_THREADS) void by_label_final_kernel(
    unsigned long long* __restrict__ tab, const unsigned long long* __restrict__ part_best, const uint32_t* __restrict__ part_cnt,
    int nparts, const uint32_t* __restrict__ set, uint32_t single, int nset, int k, int64_t row_offset,
    uint32_t* __restrict__ out_labels, float* __restrict__ out_scores, int64_t* __restrict__ out_rows, int64_t* __restrict__ out_totals,
    int32_t* __restrict__ out_count, int32_t* __restrict__ out_groups) {
  __shared__ __attribute__((aligned(16))) unsigned long long s_best[LB_MAX_SET];   // per slot, then compacted: the groups' best keys
  __shared__ unsigned long long s_tot[LB_MAX_SET];
  __shared__ unsigned long long g_best[LB_MAX_SET];
  __shared__ unsigned long long g_tot[LB_MAX_SET];
  __shared__ uint32_t g_slot[LB_MAX_SET];
  __shared__ uint32_t s_m;
  if (threadIdx.x == 0) s_m = 0;
  if (nparts > 0) {
    for (int i = threadIdx.x; i < nset; i += BL_FINAL_THREADS) {
      s_best[i] = 0ull;
      s_tot[i] = 0ull;
    }
    __syncthreads();
    const int64_t cells = (int64_t)nparts * nset;
    for (int64_t i = threadIdx.x; i < cells; i += BL_FINAL_THREADS) {
      const uint32_t c = part_cnt[i];
      if (c) {
        const int slot = (int)(i % nset);
        atomicAdd(&s_tot[slot], (unsigned long long)c);
        atomicMax(&s_best[slot], part_best[i]);
      }
    }
  } else {
    for (int i = threadIdx.x; i < nset; i += BL_FINAL_THREADS) {
      const unsigned long long c = tab[LB_MAX_SET + i];
      s_tot[i] = c;
      s_best[i] = tab[i];
      if (c) {   // zero for the next query
        tab[LB_MAX_SET + i] = 0ull;
        tab[i] = 0ull;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nset; i += BL_FINAL_THREADS) {
    if (s_tot[i]) {
      const uint32_t at = atomicAdd(&s_m, 1u);   // (any order: the rank below does not depend on it)
      g_best[at] = s_best[i];
      g_tot[at] = s_tot[i];
      g_slot[at] = (uint32_t)i;
    }
  }
  __syncthreads();
  const int m = (int)s_m;
  const int count = k < m ? (k > 0 ? k : 0) : m;
  if (threadIdx.x == 0) {
    *out_count = count;
    *out_groups = m;
  }
  if (count == 0) return;
  for (int i = threadIdx.x; i < m; i += BL_FINAL_THREADS) {
    const unsigned long long a = g_best[i];
    int above = 0;
    for (int j = 0; j < m; ++j) above += g_best[j] > a ? 1 : 0;   // one address for all lanes: a broadcast
    if (above < count) {
      out_labels[above] = nset == 1 ? single : set[g_slot[i]];
      out_scores[above] = key_score((uint32_t)(a >> 32));
      out_rows[above] = row_offset + (int64_t)(uint32_t)a;
      out_totals[above] = (int64_t)g_tot[i];
    }
  }
}

}  // namespace svs

// Group-combined search (svs_index_search_collapsed_combined): parents ranked by their best chunk PER VECTOR.
//
// Definition (include/svs_amd.h).  s_j[r] is the f32 score of row r against vector j (a single-query pass each, or the
// multi-score pass of combine.h: m score vectors, sstride floats apart).  For a group G of live rows
//     M_j(G) = max over r in G of score_key(s_j[r])                       the chunk that matches vector j best
//     c(G)   = combine.h's ONE fold over t_j = w_j * key_score(M_j(G))    MAX, MIN or the in-order SUM
//     rep(G) = the row of G with the largest make_key(c_row[r], r)        c_row: the same fold over the row's own scores
// Every reduction is a maximum of integer keys or a fixed-order f32 chain over m numbers: the answer does not depend on
// arrival order, on where a group lands in the table or on how the workgroups are scheduled.
//
// Behind the score pass, on the context's stream, with the geometry of collapse.h (strips of CL_STRIP rows, at most
// CL_GRID_MAX workgroups, the same table of tag | best-key slots, the same hash, tag scheme and probing):
//   1. cc_reduce_kernel: a thread holds four consecutive rows of all m score vectors (every load requested before the
//      first is used), folds the equal values among its four rows, and for every candidate that is left finds or claims
//      the value's slot, does ONE 64-bit atomicMax with make_key(c_row, row) on the slot's best key and m 32-bit
//      atomicMax with the per-vector keys on keys[slot * m + j] -- each behind a relaxed read that leaves the atomic out
//      when it cannot raise the value (the rows of a large group mostly lose).  No float atomics; nothing waits or spins.
//   2. cc_mark_kernel: the same stride.  An exempt row (value 0 under ZERO_SINGLE) is a group of its own: it writes the
//      fold over its own keys.  A row whose key IS its group's best writes c(G), folded from the slot's m keys.  Every
//      other row, the dead ones included, writes -inf.  All into score vector 0, which the top-k stage then reads.  The
//      survivors are counted with a ballot and one integer atomicAdd per wave.
//   3. both arrays go back to empty (all zero: no tag, and 0 is below every score key) with fills on the stream.
//   4. the top-k stage over vector 0 and collapse_values_kernel.
// Memory: the 16-byte slots of collapse.h plus 4 bytes per slot and vector, a power of two >= 2 x rows slots -- per
// million rows 2^21 slots: 32 MB + 8 MB per vector, 96 MB at m = 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "collapse.h"
#include "combine.h"

namespace svs {

// What both kernels read beside CollapseArgs: the m score vectors and weights, and the per-vector keys of every slot
struct GroupCombineArgs {
  float* scores;          // [m][sstride]; vector 0 is rewritten by the mark kernel
  int64_t sstride;        // a multiple of 4
  const float* weights;   // m
  uint32_t* keys;         // [1 << bits][m], zero = no row yet
  int m;
  int op;
};

// The slot of v, claimed if the value has none yet (the probing of collapse_insert); -1 only if every slot is another
// value's, which the capacity (>= 2 x rows) rules out
__device__ __forceinline__ int64_t cc_claim(unsigned long long* tab, int bits, uint32_t v) {
  const uint64_t mask = ((uint64_t)1 << bits) - 1;
  const unsigned long long tag = (1ull << 32) | v;
  uint64_t slot = collapse_home(v, bits);
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    unsigned long long* const t = tab + slot * CL_SLOT_WORDS;
    unsigned long long cur = __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) {
      cur = atomicCAS(t, 0ull, tag);
      if (cur == 0ull) cur = tag;
    }
    if (cur == tag) return (int64_t)slot;
    slot = (slot + 1) & mask;
  }
  return -1;
}

// The slot of v as the reduce kernel left it; -1: the value has none
__device__ __forceinline__ int64_t cc_find(const unsigned long long* tab, int bits, uint32_t v) {
  const uint64_t mask = ((uint64_t)1 << bits) - 1;
  const unsigned long long tag = (1ull << 32) | v;
  uint64_t slot = collapse_home(v, bits);
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    const unsigned long long cur = tab[slot * CL_SLOT_WORDS];
    if (cur == tag) return (int64_t)slot;
    if (cur == 0ull) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

// c over m keys: combine.h's fold applied to key_score(k_j)
template <typename F>
__device__ __forceinline__ float cc_fold(int m, int op, const float* __restrict__ weights, F key_of) {
  uint32_t acc = combine_init(op);
#pragma unroll 1
  for (int j = 0; j < m; ++j) acc = combine_step(acc, key_score(key_of(j)), weights[j], op);
  return combine_finish(acc, op);
}

// A thread's four rows of every vector: key[j][e] = score_key(s_j[row e]) for j < m, crow[e] = the row-level combined
// score (svs_index_search_combined's: the fold over the scores themselves).  j >= m: not loaded, keys 0.
struct CcRows {
  uint32_t key[CB_MAX_VECTORS][4];
  float crow[4];
  __device__ __forceinline__ CcRows(const GroupCombineArgs& g, int64_t group, bool in) {
    float4 s[CB_MAX_VECTORS];
#pragma unroll
    for (int j = 0; j < CB_MAX_VECTORS; ++j)
      s[j] = (in && j < g.m) ? ((const float4*)(g.scores + (int64_t)j * g.sstride))[group] : make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = combine_init(g.op);
#pragma unroll
    for (int j = 0; j < CB_MAX_VECTORS; ++j) {
      const float sv[4] = {s[j].x, s[j].y, s[j].z, s[j].w};
      const float w = j < g.m ? g.weights[j] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        key[j][e] = j < g.m ? score_key(sv[e]) : 0u;
        if (j < g.m) acc[e] = combine_step(acc[e], sv[e], w, g.op);   // (m is wave-uniform)
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) crow[e] = combine_finish(acc[e], g.op);
  }
};

// grid = min(strips, CL_GRID_MAX) workgroups; the table and the keys are empty on entry
__global__ __launch_bounds__(CL_THREADS) void cc_reduce_kernel(CollapseArgs a, GroupCombineArgs g) {
  using Strip = ScoredStrip<CL_THREADS, CL_VPT>;
  static_assert(CL_VPT == 1, "one group of four rows per thread and strip");
  const int64_t n4 = (a.n + 3) >> 2;
  const int64_t strips = Strip::strips(a.n);
  for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {
    const Strip s(g.scores, a.values, a.dead_bits, a.n, strip);
    CcRows rows(g, s.group(0), s.group(0) < n4);
    uint32_t vv[4];
    bool has[4];
    unsigned long long best[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      vv[e] = s.value(0, e);
      has[e] = s.live(0, e) && !(a.zero_single && vv[e] == 0u);
      best[e] = make_key(rows.crow[e], (uint32_t)s.row(0, e));
    }
    // equal values among the thread's own four rows: the latest such element carries the maxima of all of them on
#pragma unroll
    for (int e = 0; e < 3; ++e) {
#pragma unroll
      for (int f = e + 1; f < 4; ++f) {
        if (has[e] && has[f] && vv[e] == vv[f]) {
          best[f] = best[e] > best[f] ? best[e] : best[f];
#pragma unroll
          for (int j = 0; j < CB_MAX_VECTORS; ++j) rows.key[j][f] = rows.key[j][e] > rows.key[j][f] ? rows.key[j][e] : rows.key[j][f];
          has[e] = false;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!has[e]) continue;
      const int64_t slot = cc_claim(a.tab, a.bits, vv[e]);
      if (slot < 0) continue;
      unsigned long long* const b = a.tab + slot * CL_SLOT_WORDS + 1;
      // (both only grow: a read already at or above the candidate settles it without an atomic, and a stale smaller
      //  read costs one atomic that changes nothing)
      if (__hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < best[e]) atomicMax(b, best[e]);
      uint32_t* const k = g.keys + slot * g.m;
#pragma unroll
      for (int j = 0; j < CB_MAX_VECTORS; ++j)
        if (j < g.m && __hip_atomic_load(k + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < rows.key[j][e]) atomicMax(k + j, rows.key[j][e]);
    }
  }
}

// The same grid.  scores[0 .. sstride) becomes c(G) at every group's representative row and -inf everywhere else;
// *survivors (zero on entry) += the rows that stay.
__global__ __launch_bounds__(CL_THREADS) void cc_mark_kernel(CollapseArgs a, GroupCombineArgs g, unsigned long long* __restrict__ survivors) {
  using Strip = ScoredStrip<CL_THREADS, CL_VPT>;
  const int64_t n4 = (a.n + 3) >> 2;
  const int64_t strips = Strip::strips(a.n);
  uint32_t kept = 0;   // the wave's count, the same in every lane
  for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {
    const Strip s(g.scores, a.values, a.dead_bits, a.n, strip);
    const CcRows rows(g, s.group(0), s.group(0) < n4);
    float sc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = -__builtin_inff();
      bool keep = s.live(0, e);
      if (keep) {
        if (a.zero_single && s.value(0, e) == 0u) {
          sc[e] = cc_fold(g.m, g.op, g.weights, [&](int j) {
            uint32_t k = 0u;
#pragma unroll
            for (int t = 0; t < CB_MAX_VECTORS; ++t) k = t == j ? rows.key[t][e] : k;
            return k;
          });
        } else {
          const int64_t slot = cc_find(a.tab, a.bits, s.value(0, e));
          keep = slot >= 0 && a.tab[slot * CL_SLOT_WORDS + 1] == make_key(rows.crow[e], (uint32_t)s.row(0, e));
          if (keep) {
            const uint32_t* const k = g.keys + slot * g.m;
            sc[e] = cc_fold(g.m, g.op, g.weights, [&](int j) { return k[j]; });
          }
        }
      }
      kept += (uint32_t)__popcll(__ballot(keep));
    }
    if (s.group(0) < n4) ((float4*)g.scores)[s.group(0)] = make_float4(sc[0], sc[1], sc[2], sc[3]);   // (the padding past n: -inf too)
  }
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(survivors, (unsigned long long)kept);
}

}  // namespace svs

// Collapsed search (svs_index_search_collapsed): the top k rows with at most ONE row per value of a column -- "the 10
// best parent documents, each represented by its best chunk".  Values are arbitrary u32 (hashed tenant ids, 0xFFFFFFFF),
// and a corpus has as many of them as it has documents, so the groups live in an open-addressing table in HBM, not in
// LDS and not indexed by value.
//
// A group's reduction is the MAX of the order's own unique 64-bit key (keys.h: -0.0 folds onto +0.0, a NaN score is the
// largest, a score tie goes to the larger row); the number of groups is an INTEGER count.  Both are independent of
// arrival order, so the answer is exact and bit-reproducible however the workgroups are scheduled and wherever a group
// lands in the table.  Tombstoned rows leave through the dead-row BITMAP.
//
// Behind the unchanged single-query score pass, on the context's stream:
//   1. collapse_reduce_kernel: workgroups stride over strips of CL_STRIP rows; a thread's part of a strip is a
//      ScoredStrip<CL_THREADS, CL_VPT> (scored_strip.h: scores, values and tombstone bits of CL_VPT groups of four
//      consecutive rows, every load requested before the first is used).  Every live row (but a value-0 row under
//      ZERO_SINGLE) finds or claims its value's slot -- tag word 1 << 32 | v, 0 = empty, claimed with a 64-bit
//      atomicCAS, linear probing from a multiplicative hash -- and does a 64-bit atomicMax on the slot's best key.
//      Every probe either finishes or moves one slot on: no lane waits for another, nothing spins, no float atomics.
//      The capacity is a power of two >= 2 x rows, so at least half the slots stay empty and every probe sequence ends.
//      Rows of one parent usually lie next to each other: a thread first folds the equal values among its four rows,
//      then the wave folds the lanes that share its first candidate's value (wave_fold_top, shared with by_label.h) into ONE insert;
//      and an insert reads the slot's best key first and leaves the atomic out when it cannot raise it.
//   2. collapse_mark_kernel: the same stride.  A row keeps its score iff it is live and either exempt (value 0 under
//      ZERO_SINGLE) or its own key IS its group's best; every other row, the dead ones included, becomes -inf.  The
//      survivors are counted: a ballot per element, one integer atomicAdd per wave into the query's counter.
//   3. the table goes back to empty with a fill on the stream (it cannot be emptied inside the mark kernel: a tag that
//      disappears breaks the probe chain of a row that is still looking for a slot behind it).
//   4. the top-k stage over the rewritten vector, and collapse_values_kernel for the values of the returned rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"
#include "keys.h"
#include "scored_strip.h"

namespace svs {

constexpr int CL_THREADS = 256;
constexpr int CL_VPT = 1;                               // groups of four rows per thread and strip, all loaded before the first is used
constexpr int CL_STRIP = CL_THREADS * CL_VPT * 4;       // rows per strip
constexpr int CL_GRID_MAX = 1024;                       // workgroups of either kernel (four per CU: the inserts wait on L2 atomics); more rows -> more strips each
constexpr int CL_MIN_BITS = 10;                         // the smallest table: 1,024 slots
constexpr int CL_SLOT_WORDS = 2;                        // u64 words per slot: the tag, then the group's best key
constexpr int CL_ZERO_IS_GROUP = 0, CL_ZERO_SINGLE = 1; // SVS_COLLAPSE_*
static_assert(CL_STRIP % 32 == 0, "strips begin at whole bitmap words");

// What both kernels read: scores[0 .. n), the column (null: every value is 0) and the bitmap (null: no row is masked);
// the table of 1 << bits slots.
struct CollapseArgs {
  const uint32_t* values;
  const uint32_t* dead_bits;
  unsigned long long* tab;
  int64_t n;
  int bits;
  int zero_single;
};

// log2 of the capacity for n rows: the smallest power of two >= 2 n, at least 1 << CL_MIN_BITS
inline int collapse_table_bits(int64_t n) {
  int bits = CL_MIN_BITS;
  while (((int64_t)1 << bits) < 2 * n) ++bits;
  return bits;
}

__device__ __forceinline__ uint64_t collapse_home(uint32_t v, int bits) {
  return ((uint64_t)v * 0x9E3779B97F4A7C15ull) >> (64 - bits);   // (multiplicative: values i << 22 spread like any others)
}

// One group's candidate into the table.  At most one pass over the slots (it ends far earlier: half of them are empty).
__device__ __forceinline__ void collapse_insert(unsigned long long* tab, int bits, uint32_t v, unsigned long long key) {
  const uint64_t mask = ((uint64_t)1 << bits) - 1;
  const unsigned long long tag = (1ull << 32) | v;
  uint64_t slot = collapse_home(v, bits);
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    unsigned long long* const t = tab + slot * CL_SLOT_WORDS;
    // (a tag only ever goes from empty to its final value: a non-empty read is final, an empty one is settled by the CAS)
    unsigned long long cur = __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool claimed = false;
    if (cur == 0ull) {
      cur = atomicCAS(t, 0ull, tag);
      claimed = cur == 0ull;
      if (claimed) cur = tag;
    }
    if (cur == tag) {
      // (the best key only grows: a read that is already at or above this key settles it without an atomic -- the rows
      //  of a large group mostly lose --, and a stale smaller read costs one atomic that changes nothing)
      if (claimed || __hip_atomic_load(t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(t + 1, key);
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// The best key of v's group as the reduce kernel left it (0: the value has no slot)
__device__ __forceinline__ unsigned long long collapse_lookup(const unsigned long long* tab, int bits, uint32_t v) {
  const uint64_t mask = ((uint64_t)1 << bits) - 1;
  const unsigned long long tag = (1ull << 32) | v;
  uint64_t slot = collapse_home(v, bits);
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    const unsigned long long cur = tab[slot * CL_SLOT_WORDS];
    if (cur == tag) return tab[slot * CL_SLOT_WORDS + 1];
    if (cur == 0ull) return 0ull;
    slot = (slot + 1) & mask;
  }
  return 0ull;
}

// Every lane of the wave calls this (converged): has = the lane holds a candidate (value v, key).  The lanes
// that share the first candidate's value become one insert; the other candidates go in on their own.
__device__ __forceinline__ void collapse_update(unsigned long long* tab, int bits, bool has, uint32_t v, unsigned long long key) {
  const unsigned long long hit = __ballot(has);
  if (!hit) return;   // (wave-uniform)
  const uint32_t lead = (uint32_t)__shfl((int)v, __ffsll((long long)hit) - 1, 64);
  const bool peer = has && v == lead;
  bool top;
  (void)wave_fold_top(peer, (uint32_t)(key >> 32), &top);
  if (peer && !top) has = false;
  if (has) collapse_insert(tab, bits, v, key);
}

// grid = min(strips, CL_GRID_MAX) workgroups; the table is empty on entry
__global__ __launch_bounds__(CL_THREADS) void collapse_reduce_kernel(CollapseArgs a, const float* __restrict__ scores) {
  using Strip = ScoredStrip<CL_THREADS, CL_VPT>;
  const int64_t strips = Strip::strips(a.n);
  for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {   // (the trip count is the workgroup's: waves stay converged)
    const Strip s(scores, a.values, a.dead_bits, a.n, strip);
#pragma unroll
    for (int j = 0; j < CL_VPT; ++j) {
      uint32_t vv[4];
      bool has[4];
      unsigned long long key[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vv[e] = s.value(j, e);
        has[e] = s.live(j, e) && !(a.zero_single && vv[e] == 0u);
        key[e] = make_key(s.score(j, e), (uint32_t)s.row(j, e));
      }
      // equal values among the thread's own four rows: the latest such element carries the largest of their keys on
#pragma unroll
      for (int e = 0; e < 3; ++e) {
#pragma unroll
        for (int f = e + 1; f < 4; ++f) {
          if (has[e] && has[f] && vv[e] == vv[f]) {
            key[f] = key[e] > key[f] ? key[e] : key[f];
            has[e] = false;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) collapse_update(a.tab, a.bits, has[e], vv[e], key[e]);
    }
  }
}

// The same grid.  scores[r] stays for the rows of W and the exempt rows and becomes -inf for every other row;
// *survivors (zero on entry) += the rows that stay.
__global__ __launch_bounds__(CL_THREADS) void collapse_mark_kernel(CollapseArgs a, float* __restrict__ scores,
                                                                   unsigned long long* __restrict__ survivors) {
  using Strip = ScoredStrip<CL_THREADS, CL_VPT>;
  const int64_t n4 = (a.n + 3) >> 2;
  const int64_t strips = Strip::strips(a.n);
  uint32_t kept = 0;   // the wave's count, the same in every lane
  for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {
    const Strip s(scores, a.values, a.dead_bits, a.n, strip);
#pragma unroll
    for (int j = 0; j < CL_VPT; ++j) {
      float sc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[e] = s.score(j, e);
        bool keep = s.live(j, e);
        if (keep && !(a.zero_single && s.value(j, e) == 0u))
          keep = collapse_lookup(a.tab, a.bits, s.value(j, e)) == make_key(sc[e], (uint32_t)s.row(j, e));
        if (!keep) sc[e] = -__builtin_inff();
        kept += (uint32_t)__popcll(__ballot(keep));
      }
      if (s.group(j) < n4) ((float4*)scores)[s.group(j)] = make_float4(sc[0], sc[1], sc[2], sc[3]);   // (the padding past n belongs to the vector: -inf there too)
    }
  }
  if ((threadIdx.x & 63) == 0 && kept) atomicAdd(survivors, (unsigned long long)kept);
}

// out[t] = the value of returned row rows[t] (global: row_offset + local) for t < count; a column never set: 0
__global__ void collapse_values_kernel(const int64_t* __restrict__ rows, int count, int64_t row_offset, int64_t n,
                                       const uint32_t* __restrict__ values, uint32_t* __restrict__ out) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const int64_t r = rows[t] - row_offset;
    out[t] = values && r >= 0 && r < n ? values[r] : 0u;
  }
}

}  // namespace svs

// Predicate search (svs_index_search_where): the ORDERED filter of labels.h over up to WH_COLS u32 columns and a
// conjunction of up to WH_MAX_TERMS terms, on the device.
//
// The compaction IS labels.h's: where_count_kernel and where_write_kernel are its strip_count and strip_write over a
// WhereFilter, with label_scan_kernel between them and label_map_rows_kernel behind the search.  This file holds what
// the predicate adds: its filter, its loader, its terms, and the wave's ballots of "row is live and every term holds".
//
// Per step of 256 rows a lane issues ONE 16-byte load per DISTINCT column the predicate names (WhereFilter::col_mask;
// a column no term names is never read, a column the index does not own reads as 0 without a load) plus its nibble of
// the dead-row bitmap, all LB_ITERS steps' loads requested before the first is used; the four rows' terms are then
// evaluated in registers.  The column of a term is picked out of the loaded registers by compares against the
// wave-uniform column number, never by a run-time index into an array: the kernels use no scratch.
//
// The terms travel as a by-value kernel argument.  The sets of the IN terms with two members or more lie one after
// another in ONE LDS image of at most LB_MAX_SET words, each sorted and without repeats (the host's work): a term
// bisects its own slice [set0, set0 + nset) (set_floor).  A set of one member is a plain compare against WhereTerm::a (no LDS); an
// empty set is never true.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"
#include "labels.h"

namespace svs {

constexpr int WH_COLS = 4;        // SVS_COLUMNS_MAX
constexpr int WH_MAX_TERMS = 4;   // SVS_WHERE_MAX_TERMS
constexpr int WH_IN = 0, WH_RANGE = 1, WH_ANY_BITS = 2, WH_ALL_BITS = 3;   // svs_where_op

struct WhereTerm {
  uint32_t a, b;      // RANGE: a <= v <= b; ANY_BITS / ALL_BITS: the mask a; IN with nset == 1: the member a
  int32_t set0;       // IN, nset >= 2: the first word of the term's slice of the LDS image
  int32_t nset;       // IN: the distinct members
  uint32_t what;      // column | op << 8 | negate << 16 (one word: the terms are scalar registers for the whole kernel)
  __host__ __device__ int column() const { return (int)(what & 0xffu); }
  __host__ __device__ int op() const { return (int)((what >> 8) & 0xffu); }
  __host__ __device__ bool negate() const { return ((what >> 16) & 1u) != 0u; }
  static uint32_t pack(int column, int op, int negate) { return (uint32_t)column | (uint32_t)op << 8 | (uint32_t)negate << 16; }
};

// What a kernel of the filter is given: the columns (null: every value is 0), the rows, the dead-row bitmap (null when
// no row is masked), the image of the sets on the device (set_words of them; 0: no term needs LDS) and the terms.
// The columns and the terms are named members, not arrays: every access is a constant offset into the kernel argument.
struct WhereFilter {
  const uint32_t *col0, *col1, *col2, *col3;
  int64_t n;
  const uint32_t* dead_bits;
  const uint32_t* set;
  int32_t set_words;
  int32_t nterms;
  uint32_t col_mask;   // bit c: a term names column c
  WhereTerm t0, t1, t2, t3;
};
static_assert(WH_COLS == 4 && WH_MAX_TERMS == 4, "WhereFilter names four columns and four terms");

__device__ __forceinline__ void strip_stage(const WhereFilter& f, uint32_t* s_set) {
  if (f.set_words == 0) return;
  for (int i = threadIdx.x; i < f.set_words; i += LB_THREADS) s_set[i] = f.set[i];
  __syncthreads();
}

// The truth value of term t on v
__device__ __forceinline__ bool where_term(uint32_t v, const WhereTerm& t, const uint32_t* s_set) {
  bool hit;
  const int op = t.op();
  if (op == WH_RANGE) hit = t.a <= v && v <= t.b;
  else if (op == WH_ANY_BITS) hit = (v & t.a) != 0u;
  else if (op == WH_ALL_BITS) hit = (v & t.a) == t.a;
  else if (t.nset < 2) hit = t.nset == 1 && v == t.a;
  else hit = s_set[set_floor(s_set, t.set0, t.nset, v)] == v;
  return hit != t.negate();
}

// The lane's 16 bytes of a column at row i (a multiple of 4), or zeros: no term names the column, the index does not
// own it, or the rows are past the end
__device__ __forceinline__ uint4 where_load(const uint32_t* col, bool wanted, int64_t i) {
  return (wanted && col) ? ((const uint4*)col)[i >> 2] : make_uint4(0u, 0u, 0u, 0u);
}

// hit[e] &= term t on the lane's row e of the step, the term's column picked out of the step's loaded registers.
// (& and not &&: every lane evaluates every term, so the bisection's loop -- its trip count depends on nset alone --
// stays wave-uniform and no lane mask is kept across it.)
__device__ __forceinline__ void where_apply(const WhereTerm& t, const uint4 (&v)[WH_COLS], const uint32_t* s_set, bool (&hit)[4]) {
  const int col = t.column();   // (wave-uniform)
  const uint4 v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];   // (values, then selects of values: a select of the array's elements would be a run-time address)
  const bool c0 = col == 0, c1 = col == 1, c2 = col == 2;
  hit[0] = hit[0] & where_term(c0 ? v0.x : c1 ? v1.x : c2 ? v2.x : v3.x, t, s_set);
  hit[1] = hit[1] & where_term(c0 ? v0.y : c1 ? v1.y : c2 ? v2.y : v3.y, t, s_set);
  hit[2] = hit[2] & where_term(c0 ? v0.z : c1 ? v1.z : c2 ? v2.z : v3.z, t, s_set);
  hit[3] = hit[3] & where_term(c0 ? v0.w : c1 ? v1.w : c2 ? v2.w : v3.w, t, s_set);
}

// The calling wave's part of strip `blockIdx.x`: b[j][e] = the ballot of "row row0 + 256 j + 4 lane + e matches";
// returns the wave's matches.  row0 (out) = the wave's first row.  load_mask (wave-uniform, a superset of f.col_mask):
// bit c = column c is loaded; v[j][c] (out) = the lane's four values of column c at step j, zeros where it was not.
__device__ __forceinline__ int where_ballots(const WhereFilter& f, uint32_t load_mask, const uint32_t* s_set,
                                             unsigned long long (&b)[LB_ITERS][4], uint4 (&v)[LB_ITERS][WH_COLS], int64_t* row0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * LB_STRIP + (int64_t)wave * LB_WAVE_ROWS;
  *row0 = w0;
  uint32_t dead[LB_ITERS];
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {   // all requested before the first is used
    const int64_t i = w0 + j * 256 + lane * 4;   // a multiple of 4: one 16-byte load per column, one nibble of a bitmap word
    const bool in = i < f.n;
    v[j][0] = where_load(f.col0, in && (load_mask & 1u), i);
    v[j][1] = where_load(f.col1, in && (load_mask & 2u), i);
    v[j][2] = where_load(f.col2, in && (load_mask & 4u), i);
    v[j][3] = where_load(f.col3, in && (load_mask & 8u), i);
    dead[j] = dead_nibble(in ? f.dead_bits : nullptr, i >> 2);
  }
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {
    const int64_t i = w0 + j * 256 + lane * 4;
    bool hit[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) hit[e] = i + e < f.n && !((dead[j] >> e) & 1u);
    if (f.nterms > 0) where_apply(f.t0, v[j], s_set, hit);   // (wave-uniform)
    if (f.nterms > 1) where_apply(f.t1, v[j], s_set, hit);
    if (f.nterms > 2) where_apply(f.t2, v[j], s_set, hit);
    if (f.nterms > 3) where_apply(f.t3, v[j], s_set, hit);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      b[j][e] = __ballot(hit[e]);
      cnt += __popcll(b[j][e]);
    }
  }
  return cnt;
}

// strip_count's and strip_write's view of it: the columns the terms name.  (The payload is the row: nothing is left in
// the uint4s.)
__device__ __forceinline__ int strip_ballots(const WhereFilter& f, const uint32_t* s_set, unsigned long long (&b)[LB_ITERS][4],
                                             uint4 (&)[LB_ITERS], int64_t* row0) {
  uint4 v[LB_ITERS][WH_COLS];
  return where_ballots(f, f.col_mask, s_set, b, v, row0);
}

// grid = ceil(n / LB_STRIP) workgroups.  counts[blockIdx.x] = the strip's matches; *total += them (zero on entry).
__global__ __launch_bounds__(LB_THREADS) void where_count_kernel(WhereFilter f, uint32_t* __restrict__ counts,
                                                                 unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ int s_wave[LB_WAVES];
  strip_count(f, s_set, s_wave, counts, total);
}

// grid as where_count_kernel, same filter.  bases = the scanned counts; out[0 .. m) receives the matching local rows in
// ascending order.  m = the total the count pass found: a slot at or past it is never written.
__global__ __launch_bounds__(LB_THREADS) void where_write_kernel(WhereFilter f, const uint32_t* __restrict__ bases,
                                                                 uint32_t* __restrict__ out, int64_t m) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ int s_wave[LB_WAVES];
  strip_write<LB_ROWS>(f, s_set, s_wave, bases, out, m);
}

}  // namespace svs

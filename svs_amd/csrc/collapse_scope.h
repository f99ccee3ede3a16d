// Collapsed search inside a scope (svs_index_search_collapsed_where, svs_index_search_collapsed_rows): collapse.h's
// groups over the rows S of a predicate or of a row list instead of over every live row.
//
// gather.h scores a device list of rows into a COMPACT vector: position p holds the score of row list[p].  collapse.h's
// kernels walk a score vector with the group column beside it in the SAME index space, so the one thing the scoped
// search needs is the group column compacted the same way: cvals[p] = column[list[p]].  With that, collapse_reduce_kernel
// and collapse_mark_kernel run unchanged over the m = |S| positions -- no bitmap (S holds live rows only), a table sized
// by m --, the top-k stage ranks positions, and label_map_rows_kernel turns them into rows.  The list ascends, so
// positions ascend with rows and make_key(score, position) orders a group's rows as make_key(score, row) does: a score
// tie goes to the larger row.
//
//   scoped_write_kernel   the write pass of where.h with two outputs from ONE evaluation of the predicate: the row list
//                         and the compacted group column.  The group column is one more 16-byte load per lane and step,
//                         requested with the predicate's columns (where_ballots' load_mask); a column a term names
//                         anyway is loaded once; a column the index does not own is not loaded and writes 0.  The
//                         value is picked out of the loaded registers by compares against the wave-uniform column
//                         number: no scratch.
//   scoped_values_kernel  the same column for a list that came from the host (svs_index_search_collapsed_rows).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "labels.h"
#include "where.h"

namespace svs {

// grid as where_count_kernel, same filter.  bases = the scanned counts, m = the total the count pass found.
// list[0 .. m) receives the matching local rows in ascending order, cvals[0 .. m) their values of column gcol
// (0 .. WH_COLS - 1).  A slot at or past m is never written.
__global__ __launch_bounds__(LB_THREADS) void scoped_write_kernel(WhereFilter f, int gcol, const uint32_t* __restrict__ bases,
                                                                  uint32_t* __restrict__ list, uint32_t* __restrict__ cvals, int64_t m) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ int s_wave[LB_WAVES];
  strip_stage(f, s_set);
  unsigned long long b[LB_ITERS][4];
  uint4 v[LB_ITERS][WH_COLS];
  int64_t row0;
  const int cnt = where_ballots(f, f.col_mask | 1u << gcol, s_set, b, v, &row0);
  const bool c0 = gcol == 0, c1 = gcol == 1, c2 = gcol == 2;   // (wave-uniform)
  uint4 g[LB_ITERS];
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {   // (selects of values: a select of the array's elements would be a run-time address)
    const uint4 v0 = v[j][0], v1 = v[j][1], v2 = v[j][2], v3 = v[j][3];
    g[j] = make_uint4(c0 ? v0.x : c1 ? v1.x : c2 ? v2.x : v3.x, c0 ? v0.y : c1 ? v1.y : c2 ? v2.y : v3.y,
                      c0 ? v0.z : c1 ? v1.z : c2 ? v2.z : v3.z, c0 ? v0.w : c1 ? v1.w : c2 ? v2.w : v3.w);
  }
  const int lane = threadIdx.x & 63;
  strip_slots(b, cnt, s_wave, bases, m, [&](int64_t s, int j, int e) {
    list[s] = (uint32_t)(row0 + j * 256 + lane * 4 + e);
    cvals[s] = uint4_at(g[j], e);
  });
}

// cvals[p] = values[list[p]] for p < m (values null: the index does not own the column, every value is 0)
__global__ __launch_bounds__(256) void scoped_values_kernel(const uint32_t* __restrict__ list, int64_t m,
                                                            const uint32_t* __restrict__ values, uint32_t* __restrict__ cvals) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x)
    cvals[p] = values ? values[list[p]] : 0u;
}

}  // namespace svs

// Segmented filtered search (svs_index_search_segments): MANY row lists in one call, each scored against its own query
// and ranked on its own -- the drill-down of a document tree (one query, one list per parent) and per-request scopes
// (one list per query).  Segment s's answer is svs_index_search_rows' answer for (its query, its list), bit for bit;
// nothing is merged across segments.
//
// Host plan (seg_tile_plan, pure host code): the live rows of every segment of 1 .. SORT_CAP rows are concatenated as
// local u32 rows into ONE list, and a tile table is laid beside it.  A tile is the work of one WAVE of the score kernel,
// W = (64 / T) U rows with the geometry of gather.h: {list offset (= score offset), rows in the tile, query}.  A tile
// never spans two segments, so everything a wave needs besides its rows is wave-uniform (scalar registers, one 16-byte
// load), and a segment of m rows costs ceil(m / W) waves wherever it lies in the call.  Tiles are per WAVE and not per
// workgroup because the lists of a drill-down are short: a workgroup takes 8 to 8192 rows depending on the row length,
// and at one segment per workgroup a call of 256 lists of 100 rows would leave most waves of the launch idle for short
// rows; at one tile per wave only the last wave of each segment is ragged.  Segments of more than SORT_CAP live rows
// take svs_index_search_rows' own kernels.
//
// gather_segments_kernel: gather_wave (gather.h), the one-query body of gather_scores_kernel, driven by the tile table:
// the same function, so a row's score has the same bits as there.  Lanes past the tile's rows re-read the tile's own
// last list entry and store nothing (the next score belongs to another segment).  No LDS, no barrier; HBM-bound like
// gather_scores_kernel: bytes = listed rows x row bytes.
//
// select_segments_kernel: one workgroup per segment sorts make_key(score, position) of its <= SORT_CAP scores in LDS
// (select_final_kernel's mode 1: rank emission up to FINAL_THREADS keys, the bitonic network beyond) and writes
// count_s results at stride kk with the row mapped ON THE DEVICE, row_offset + list[position]: each segment's list is
// ascending, so "position desc" is "row desc" (gather.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gather.h"
#include "select.h"

namespace svs {

// One wave's work: rows list[off .. off + rows) of ONE segment against staged query `query`; scores[off + p]
struct SegTile {
  uint32_t off, rows, query, seg;
};
// One small segment: its m scores / list entries from `off`, `count` results wanted; `seg` = its number in the call
struct SegDesc {
  uint32_t off, m, count, seg;
};
static_assert(sizeof(SegTile) == 16 && sizeof(SegDesc) == 16, "one 16-byte load each");

// The tile table of a call, pure host code.  sizes[nseg]: live rows per segment; seg_query[nseg] or null (segment s
// takes query s); w: rows per wave.  Segments of 1 .. SORT_CAP rows get ceil(m / w) tiles at consecutive list offsets in
// segment order; empty and larger segments get none.  seg_off[nseg] (may be null): a small segment's list offset, -1
// for the others.  Up to cap tiles are written (tiles may be null when cap == 0).  Returns the number of tiles, or -1
// when the small segments hold 2^31 rows or more (*total_rows, may be null, gets their sum either way).
inline int64_t seg_tile_plan(const int64_t* sizes, const int32_t* seg_query, int64_t nseg, int64_t w, SegTile* tiles, int64_t cap,
                             int64_t* seg_off, int64_t* total_rows) {
  int64_t off = 0, nt = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t m = sizes[s];
    const bool small = m >= 1 && m <= SORT_CAP;
    if (seg_off) seg_off[s] = small ? off : -1;
    if (!small) continue;
    if (off + m < ((int64_t)1 << 31)) {
      for (int64_t p = 0; p < m; p += w, ++nt)
        if (nt < cap)
          tiles[nt] = SegTile{(uint32_t)(off + p), (uint32_t)(m - p < w ? m - p : w), (uint32_t)(seg_query ? seg_query[s] : s), (uint32_t)s};
    }
    off += m;
  }
  if (total_rows) *total_rows = off;
  return off < ((int64_t)1 << 31) ? nt : -1;
}

// M, ld16, row_scales, q_scales: as gather_scores_kernel; list: the concatenated local rows; q: the call's staged
// queries, [nq][ld16]; wave w of the grid takes tiles[w].
template <int DT, int T, int NC, int U>
__global__ __launch_bounds__(gather_wpb(NC) * 64) void gather_segments_kernel(
    const u32x4* __restrict__ M, int ld16, const uint32_t* __restrict__ list, const SegTile* __restrict__ tiles, int64_t ntiles,
    const u32x4* __restrict__ q, const float* __restrict__ row_scales, const float* __restrict__ q_scales,
    float* __restrict__ scores) {
  constexpr int WPB = gather_wpb(NC);
  const int64_t w = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (w >= ntiles) return;
  const SegTile tile = tiles[w];
  // (the same for every lane of the wave: kept in scalar registers)
  const uint32_t off = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile.off);
  const int nrows = __builtin_amdgcn_readfirstlane((int)tile.rows);
  const uint32_t qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile.query);
  gather_wave<DT, T, NC, U, false>(M, ld16, list + off, nrows, q + (size_t)qi * ld16, 1, row_scales, q_scales + qi, scores + off, 0);
}

// grid = the call's small segments; out_scores / out_rows: [segments][kk], entries past a segment's count untouched
__global__ __launch_bounds__(FINAL_THREADS) void select_segments_kernel(
    const float* __restrict__ scores, const uint32_t* __restrict__ list, const SegDesc* __restrict__ segs, int kk,
    int64_t row_offset, float* __restrict__ out_scores, int64_t* __restrict__ out_rows) {
  __shared__ __attribute__((aligned(16))) uint64_t S[SORT_CAP];
  const SegDesc sd = segs[blockIdx.x];
  const float* s = scores + sd.off;
  const uint32_t* rows = list + sd.off;
  const int n = (int)sd.m, count = (int)sd.count;
  float* os = out_scores + (int64_t)blockIdx.x * kk;
  int64_t* orow = out_rows + (int64_t)blockIdx.x * kk;
  const int m = next_pow2(n < 2 ? 2 : n);
  for (int i = threadIdx.x; i < m; i += blockDim.x) S[i] = i < n ? make_key(s[i], (uint32_t)i) : 0ull;
  __syncthreads();
  if (m <= FINAL_THREADS) {
    // one key per thread: its place is the number of keys above it (emit_by_rank; a real key is never 0)
    const uint64_t a = (int)threadIdx.x < m ? S[threadIdx.x] : 0ull;
    const ulonglong2* S2 = reinterpret_cast<const ulonglong2*>(S);
    int above = 0;
#pragma unroll 4
    for (int j = 0; j < (m >> 1); ++j) {
      const ulonglong2 p = S2[j];
      above += (p.x > a ? 1 : 0) + (p.y > a ? 1 : 0);
    }
    if (a != 0ull && above < count) {
      os[above] = key_score((uint32_t)(a >> 32));
      orow[above] = row_offset + (int64_t)rows[(uint32_t)a];
    }
  } else {
    bitonic_sort_lds_desc(S, m);
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
      const uint64_t key = S[i];
      os[i] = key_score((uint32_t)(key >> 32));
      orow[i] = row_offset + (int64_t)rows[(uint32_t)key];
    }
  }
}

}  // namespace svs

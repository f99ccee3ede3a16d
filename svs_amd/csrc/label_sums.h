// Per-label row sums (svs_index_label_sums): for every label of a caller-given set, the f64 sum of the stored values
// of the live rows of a range that carry it, and how many there are -- the update step of k-means beside
// svs_index_assign, and a label's centroid without pulling its rows out of HBM.
//
// The sum is DEFINED as a fixed tree (include/svs_amd.h): a label's live rows in ascending order are cut into chunks of
// LS_CHUNK = 256; a chunk is ONE chain of f64 additions over its rows starting from +0.0, a label's sum ONE chain over
// its chunks' partial sums starting from +0.0.  So rows must reach the adder in row order, which an atomic scatter-add
// cannot give: the kernels build, per call, an inverted index -- a label-major list of the matching rows, ascending
// within a label -- and sum along it.  Six launches on the context's stream, no host wait in between:
//
//   1. label_sums_hist_kernel     One workgroup per strip of LS_STRIP consecutive rows of the range.  A row's label (the
//                                 column, the call's row_labels, or 0) is searched in the set's LDS image
//                                 (label_stage_set, label_slot); live rows by the bitmap.  An LDS table of u32 counts
//                                 (integer LDS atomics: order-free) goes out whole as hist[strip][slot].
//   2. label_sums_scan_kernel     One workgroup per slot: the strips' counts of the slot become their exclusive prefix
//                                 sums in place (block_run_scan, as label_scan_kernel); tot[slot] = the label's rows.  A
//                                 count-only call ends here.
//   3. label_sums_plan_kernel     One workgroup: scans over the slots give each label's first list position and first
//                                 chunk; then the chunk table, one entry (slot, first list position, length <= 256) per
//                                 chunk.  Chunks never cross a label.  Entries from the last chunk up to the grid bound
//                                 ceil(nrows / 256) + nset get length 0: their workgroups exit.
//   4. label_sums_scatter_kernel  Strips as in 1.  Wave w owns rows 256 w .. 256 w + 255 of the strip and takes them in
//                                 four steps of 64, so (wave, step, lane) order IS row order.  Per-wave counts (LDS
//                                 atomics) turn into per-wave bases: strip base + the earlier waves.  Then each wave
//                                 walks its steps in order; per distinct slot of a step ONE lane takes the slot's
//                                 running counter (an LDS add that returns the old value, in program order), and a
//                                 lane's rank is that plus the matching lanes below it.  Positions ascend with the rows.
//   5. label_sums_chunk_kernel<DT>  grid (chunk bound, column blocks of 256 16-byte pieces).  The chunk's list entries go
//                                 to LDS first; wave w then owns 64 consecutive 16-byte pieces of the row (a 1 KiB
//                                 coalesced load per row, 64-bit addressing row * ld16), LS_U rows requested before the
//                                 first is added.  decode_chunk<DT> (chunk.h), fp8 times the row's scale as one f32
//                                 product -- dequant_rows_fp8_kernel's value --, widened to f64 (exact) and added to
//                                 f64 accumulators in registers in list order.  partial[chunk][col], f64.
//   6. label_sums_fold_kernel     Per (slot, column): the label's partials in ascending chunk order, one chain from
//                                 +0.0, into the (nset, d) output image.  One D2H copy follows.
//
// Nothing is fused or reassociated (fp contraction is off in 5 and 6; no multiply meets an add anyway), no float
// atomics, no workgroup waits for or spins on another, plain vector stores.  Every row number is clamped into [0, n)
// before it addresses anything; list positions are checked against the label's count and the list's length, chunk
// entries against the list's length, the fold's chunk range against the table's.
// Local rows and the strips' prefixes are u32: a handle holds fewer than 2^32 rows (ensure_capacity; the host entry checks).
// Floors: 1 and 4 read 4 bytes of label and one bit per row (launch-bound); 5 reads every matching row once -- the
// HBM-read floor of a single-query score pass over those rows -- and writes (chunks x d) f64; 6 reads that back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chunk.h"
#include "labels.h"

namespace svs {

constexpr int LS_THREADS = 256;
constexpr int LS_WAVES = LS_THREADS / 64;
constexpr int LS_STEPS = 4;                            // rows per lane and strip
constexpr int LS_WAVE_ROWS = 64 * LS_STEPS;            // consecutive rows a wave owns
constexpr int LS_STRIP = LS_WAVES * LS_WAVE_ROWS;      // rows per strip
constexpr int LS_CHUNK = 256;                          // SVS_LABEL_SUMS_CHUNK: rows of one partial sum
constexpr int LS_U = 8;                                // rows in flight per wave in the chunk kernel
constexpr int LS_PLAN_THREADS = 1024;
constexpr int LS_FOLD_THREADS = 64;
static_assert(LS_THREADS == LB_THREADS, "label_stage_set strides by LB_THREADS");
static_assert(LS_PLAN_THREADS == LB_MAX_SET, "the plan kernel scans the slots one per thread");
static_assert(LS_CHUNK <= LS_THREADS, "the chunk kernel stages a chunk's list entries one per thread");

struct LsChunk {          // one entry of the chunk table
  uint32_t slot;
  uint32_t len;           // 0: past the last chunk
  unsigned long long first;   // list position of the chunk's first row
};

// The range: local rows [r0, r0 + nrows) of the f.n rows the index holds.  row_labels: null, or the range's labels
// (nrows of them) in place of the column.
struct LsRange {
  int64_t r0, nrows;
  const uint32_t* row_labels;
};

// The slot of range row i (relative to r0), or -1: outside the range, tombstoned, or a label that is not in the set
__device__ __forceinline__ int label_sums_slot(const LabelFilter& f, const LsRange& g, const uint32_t* s_set, int64_t i) {
  if (i >= g.nrows) return -1;
  int64_t row = g.r0 + i;
  row = row < 0 ? 0 : (row < f.n ? row : f.n - 1);
  if (row_dead(f.dead_bits, row)) return -1;
  const uint32_t v = g.row_labels ? g.row_labels[i] : (f.labels ? f.labels[row] : 0u);
  return label_slot(v, f, s_set);
}

// grid = ceil(nrows / LS_STRIP).  hist[blockIdx.x * f.nset + slot] = the strip's live rows of the slot's label.
__global__ __launch_bounds__(LS_THREADS) void label_sums_hist_kernel(LabelFilter f, LsRange g, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ uint32_t s_cnt[LB_MAX_SET];
  for (int i = threadIdx.x; i < f.nset; i += LS_THREADS) s_cnt[i] = 0u;
  label_stage_set(f, s_set);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * LS_STRIP + (int64_t)wave * LS_WAVE_ROWS;
  int slot[LS_STEPS];
#pragma unroll
  for (int j = 0; j < LS_STEPS; ++j) slot[j] = label_sums_slot(f, g, s_set, w0 + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < LS_STEPS; ++j)
    if (slot[j] >= 0) atomicAdd(&s_cnt[slot[j]], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < f.nset; i += LS_THREADS) hist[(int64_t)blockIdx.x * f.nset + i] = s_cnt[i];
}

// grid = nset, one workgroup per slot.  hist[strip * nset + slot], strip < nstrips -> its exclusive prefix sum over the
// strips, in place (block_run_scan at stride nset; a prefix is below the range's rows, at most 2^32); tot[slot] = the sum.
__global__ __launch_bounds__(LS_THREADS) void label_sums_scan_kernel(uint32_t* __restrict__ hist, int64_t nstrips, int nset,
                                                                     unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long s_sum[LS_THREADS];
  const unsigned long long total = block_run_scan<LS_THREADS>(hist + blockIdx.x, nstrips, nset, s_sum);
  if (threadIdx.x == LS_THREADS - 1) tot[blockIdx.x] = total;
}

// One workgroup.  tot[0 .. nset) -> lbase[slot] = the list position of the label's first row, cbase[slot] = its first
// chunk (cbase[nset] = the chunks in all), table[0 .. bound): the chunks, then entries of length 0.
__global__ __launch_bounds__(LS_PLAN_THREADS) void label_sums_plan_kernel(const unsigned long long* __restrict__ tot, int nset,
                                                                          unsigned long long* __restrict__ lbase,
                                                                          unsigned long long* __restrict__ cbase,
                                                                          LsChunk* __restrict__ table, int64_t bound) {
  __shared__ unsigned long long s_l[LS_PLAN_THREADS];   // inclusive scans: rows, chunks
  __shared__ unsigned long long s_c[LS_PLAN_THREADS];
  __shared__ unsigned long long s_n[LS_PLAN_THREADS];   // the labels' rows
  const int t = threadIdx.x;
  const unsigned long long cnt = t < nset ? tot[t] : 0ull;
  const unsigned long long nch = (cnt + LS_CHUNK - 1) / LS_CHUNK;
  s_l[t] = cnt;
  s_c[t] = nch;
  s_n[t] = cnt;
  unsigned long long* const both[2] = {s_l, s_c};
  block_scan<LS_PLAN_THREADS>(both);
  if (t < nset) {
    lbase[t] = s_l[t] - cnt;
    cbase[t] = s_c[t] - nch;
  }
  const unsigned long long total = s_c[LS_PLAN_THREADS - 1];
  if (t == 0) cbase[nset] = total;
  for (int64_t c = t; c < bound; c += LS_PLAN_THREADS) {
    LsChunk e{0u, 0u, 0ull};
    if ((unsigned long long)c < total) {
      int lo = 0, len = nset;   // the first slot whose inclusive chunk count exceeds c: the chunk's label
      while (len > 0) {
        const int half = len >> 1;
        if (s_c[lo + half] <= (unsigned long long)c) { lo += half + 1; len -= half + 1; }
        else len = half;
      }
      lo = lo < nset ? lo : nset - 1;
      const unsigned long long k = (unsigned long long)c - (s_c[lo] - (s_n[lo] + LS_CHUNK - 1) / LS_CHUNK);   // the chunk within its label
      const unsigned long long left = s_n[lo] - k * LS_CHUNK;
      e.slot = (uint32_t)lo;
      e.len = k * LS_CHUNK < s_n[lo] ? (uint32_t)(left < LS_CHUNK ? left : LS_CHUNK) : 0u;
      e.first = s_l[lo] - s_n[lo] + k * LS_CHUNK;
    }
    table[c] = e;
  }
}

// grid and filter as label_sums_hist_kernel; hist = the scanned counts, lbase / tot as the plan kernel left them.
// list[0 .. list_len): per label from lbase[slot] on, its live rows of the range as LOCAL rows (r0 + i), ascending.
__global__ __launch_bounds__(LS_THREADS) void label_sums_scatter_kernel(LabelFilter f, LsRange g, const uint32_t* __restrict__ hist,
                                                                        const unsigned long long* __restrict__ lbase,
                                                                        const unsigned long long* __restrict__ tot,
                                                                        uint32_t* __restrict__ list, int64_t list_len) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ uint32_t s_run[LS_WAVES][LB_MAX_SET];   // per wave: first its counts, then its running rank within the label
  for (int i = threadIdx.x; i < LS_WAVES * f.nset; i += LS_THREADS) s_run[i / f.nset][i % f.nset] = 0u;
  label_stage_set(f, s_set);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * LS_STRIP + (int64_t)wave * LS_WAVE_ROWS;
  int slot[LS_STEPS];
#pragma unroll
  for (int j = 0; j < LS_STEPS; ++j) slot[j] = label_sums_slot(f, g, s_set, w0 + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < LS_STEPS; ++j)
    if (slot[j] >= 0) atomicAdd(&s_run[wave][slot[j]], 1u);
  __syncthreads();
  for (int i = threadIdx.x; i < f.nset; i += LS_THREADS) {   // counts -> bases: the strip's, then the earlier waves
    uint32_t b = hist[(int64_t)blockIdx.x * f.nset + i];
#pragma unroll
    for (int w = 0; w < LS_WAVES; ++w) {
      const uint32_t c = s_run[w][i];
      s_run[w][i] = b;
      b += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LS_STEPS; ++j) {
    unsigned long long todo = __ballot(slot[j] >= 0);   // (wave-uniform: the loop below is too)
    while (todo) {
      const int lead_lane = __ffsll((long long)todo) - 1;
      const int lead = __shfl(slot[j], lead_lane, 64);
      const unsigned long long peers = __ballot(slot[j] == lead);
      uint32_t base = 0u;
      if (lane == lead_lane) base = atomicAdd(&s_run[wave][lead], (uint32_t)__popcll(peers));   // one grab per (wave, step, slot), in program order
      base = (uint32_t)__shfl((int)base, lead_lane, 64);
      if (slot[j] == lead) {
        const unsigned long long rank = (unsigned long long)base + (unsigned long long)__popcll(peers & ((1ull << lane) - 1ull));
        const unsigned long long pos = lbase[lead] + rank;
        if (rank < tot[lead] && pos < (unsigned long long)list_len) list[pos] = (uint32_t)(g.r0 + w0 + j * 64 + lane);
      }
      todo &= ~peers;
    }
  }
}

// grid = (chunk bound, ceil(ld16 / LS_THREADS)).  M: n rows of ld16 16-byte pieces (DT: 0 f32, 1 f16, 2 fp8).
// partial[chunk * d + col] = the chain over the chunk's rows, col < d.
template <int DT>
__global__ __launch_bounds__(LS_THREADS) void label_sums_chunk_kernel(const u32x4* __restrict__ M, int ld16, const float* __restrict__ row_scales,
                                                                      int64_t n, int d, const LsChunk* __restrict__ table,
                                                                      const uint32_t* __restrict__ list, int64_t list_len,
                                                                      double* __restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int EPC = elems_per_chunk(DT);
  __shared__ uint32_t s_rows[LS_CHUNK];
  const LsChunk e = table[blockIdx.x];
  const int len = e.len <= (uint32_t)LS_CHUNK ? (int)e.len : 0;
  if (len == 0 || e.first + (unsigned long long)len > (unsigned long long)list_len) return;   // (workgroup-uniform)
  if ((int)threadIdx.x < len) {
    int64_t row = (int64_t)list[e.first + threadIdx.x];
    s_rows[threadIdx.x] = (uint32_t)(row < n ? row : n - 1);
  }
  __syncthreads();
  const int piece = blockIdx.y * LS_THREADS + threadIdx.x;
  if ((piece & ~63) >= ld16) return;   // (wave-uniform; nothing synchronises below)
  const bool mine = piece < ld16;
  const u32x4* src = M + (mine ? piece : ld16 - 1);
  double acc[EPC];
#pragma unroll
  for (int k = 0; k < EPC; ++k) acc[k] = 0.0;
  for (int i0 = 0; i0 < len; i0 += LS_U) {
    u32x4 buf[LS_U];
    float sc[LS_U];
#pragma unroll
    for (int u = 0; u < LS_U; ++u) {   // all requested before the first is added
      const int64_t row = (int64_t)s_rows[i0 + u < len ? i0 + u : len - 1];
      buf[u] = src[row * ld16];
      sc[u] = DT == 2 ? row_scales[row] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < LS_U; ++u) {
      if (i0 + u < len) {   // (wave-uniform)
        float v[EPC];
        decode_chunk<DT>(buf[u], v);
#pragma unroll
        for (int k = 0; k < EPC; ++k) {
          float x = v[k];
          if constexpr (DT == 2) x = x * sc[u];   // one f32 product: the stored value
          acc[k] = acc[k] + (double)x;
        }
      }
    }
  }
  if (mine) {
    double* o = partial + (int64_t)blockIdx.x * d + (int64_t)piece * EPC;
#pragma unroll
    for (int k = 0; k < EPC; ++k)
      if (piece * EPC + k < d) o[k] = acc[k];
  }
}

// grid = (ceil(d / LS_FOLD_THREADS), nset).  out[slot * d + col] = the chain over the label's partials in chunk order.
__global__ __launch_bounds__(LS_FOLD_THREADS) void label_sums_fold_kernel(const double* __restrict__ partial, const unsigned long long* __restrict__ tot,
                                                                          const unsigned long long* __restrict__ cbase, int d, int64_t bound,
                                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
  const int slot = blockIdx.y, col = blockIdx.x * LS_FOLD_THREADS + threadIdx.x;
  if (col >= d) return;
  const unsigned long long c0 = cbase[slot];
  unsigned long long nch = (tot[slot] + LS_CHUNK - 1) / LS_CHUNK;
  if (c0 >= (unsigned long long)bound) nch = 0;
  else if (nch > (unsigned long long)bound - c0) nch = (unsigned long long)bound - c0;
  const double* p = partial + (int64_t)c0 * d + col;
  double acc = 0.0;
  for (unsigned long long t = 0; t < nch; ++t) acc = acc + p[(int64_t)t * d];
  out[(int64_t)slot * d + col] = acc;
}

}  // namespace svs

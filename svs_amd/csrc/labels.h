// Labelled search (svs_index_search_labeled) and the label column's compaction: an ORDERED filter over the index's
// one-u32-per-row label column, on the device.
//
// The filter is a two-pass stream compaction over fixed strips of LB_STRIP consecutive rows, one workgroup per strip:
//   1. label_count_kernel: evaluates the predicate "row is live and its label is in the set" for the strip, counts the
//      matches per wave (__ballot + __popcll), writes ONE count per workgroup and adds it to the call's total.
//   2. label_scan_kernel, one workgroup: the counts become exclusive prefix sums in place -- the base of every strip.
//   3. label_write_kernel<PAYLOAD>: evaluates the predicate again; a match's slot is the strip's base + the matches in
//      the earlier waves of the strip + the matches before it in its own wave (mbcnt of the wave's ballots).  Slots
//      ascend with the rows, so the output is the matches in strictly ascending row order: the device row list
//      enqueue_list_search takes (PAYLOAD 0, the row index) or the compacted label column (PAYLOAD 1, the label value).
// The two passes are written once, as strip_count and strip_write<PAYLOAD>, for every filter type over strips
// (LabelFilter here, WhereFilter in where.h): the type's overloads of strip_stage and strip_ballots stage its LDS image
// and give the calling wave's ballots for the strip.  The __global__ kernels own the LDS arrays and call one of the two.
// No workgroup ever waits for another: the only thing that crosses workgroups is the per-strip count, and it crosses
// through a kernel boundary.  Every label is read twice per call (once per pass): a 1M-row column is 4 MB, the kernels
// are launch-bound.
//
// A wave owns LB_WAVE_ROWS consecutive rows of the strip and takes them in LB_ITERS steps of 256: lane l loads the four
// labels of rows 4 l .. 4 l + 3 of the step as one 16-byte load (a wave's step is one 1 KiB load), and the four rows'
// tombstone bits are one nibble of the dead-row bitmap.  The set, sorted and without repeats, sits in LDS (4 KiB at
// most) and is searched by bisection per row; a set of ONE label is a kernel argument and a plain compare, with no LDS;
// an EMPTY set means "every label" (the compaction's predicate is "row is live" alone).
//
// label_map_rows_kernel: after run_select has written list POSITIONS (enqueue_list_search), positions -> global rows
// on the device, because the list never exists on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dead_bits.h"

namespace svs {

constexpr int LB_THREADS = 256;
constexpr int LB_WAVES = LB_THREADS / 64;
constexpr int LB_ITERS = 2;                           // 16-byte label loads per lane, all requested before the first is used
constexpr int LB_WAVE_ROWS = 64 * 4 * LB_ITERS;       // consecutive rows a wave owns
constexpr int LB_STRIP = LB_WAVES * LB_WAVE_ROWS;     // rows per workgroup strip (a multiple of 32: whole bitmap words)
constexpr int LB_MAX_SET = 1024;                      // SVS_LABELS_MAX_SET: the set's LDS image is 4 KiB at most
constexpr int LB_ROWS = 0, LB_VALUES = 1;             // label_write_kernel's payload

// What a kernel of the filter is given: the column (null: every label is 0), the rows it covers, the dead-row bitmap
// (dead_bits.h; null when no row is masked), and the set -- nset == 0: every label matches; nset == 1:
// `single`; nset >= 2: set[0 .. nset) on the device, strictly ascending.
struct LabelFilter {
  const uint32_t* labels;
  int64_t n;
  const uint32_t* dead_bits;
  const uint32_t* set;
  int nset;
  uint32_t single;
};

// nset >= 2: the workgroup's copy of the set (call it from every thread, before strip_ballots)
__device__ __forceinline__ void label_stage_set(const LabelFilter& f, uint32_t* s_set) {
  if (f.nset < 2) return;
  for (int i = threadIdx.x; i < f.nset; i += LB_THREADS) s_set[i] = f.set[i];
  __syncthreads();
}

// Bisection of the sorted slice s_set[lo .. lo + len), len >= 1, of an LDS image: where the last entry <= v is, if there
// is one (the caller compares).  The trip count depends on len alone.
__device__ __forceinline__ int set_floor(const uint32_t* s_set, int lo, int len, uint32_t v) {
  while (len > 1) {   // the last entry <= v, if there is one, is in [lo, lo + len)
    const int half = len >> 1;
    lo = s_set[lo + half] <= v ? lo + half : lo;
    len -= half;
  }
  return lo;
}

// The SLOT of v, its index in the sorted set (nset >= 1), or -1: one label a compare, more a bisection of the LDS image
__device__ __forceinline__ int label_slot(uint32_t v, const LabelFilter& f, const uint32_t* s_set) {
  int at = 0;
  bool hit;
  if (f.nset == 1) hit = v == f.single;
  else {
    at = set_floor(s_set, 0, f.nset, v);
    hit = s_set[at] == v;
  }
  return hit ? at : -1;
}

__device__ __forceinline__ bool label_in_set(uint32_t v, const LabelFilter& f, const uint32_t* s_set) {
  return f.nset == 0 || label_slot(v, f, s_set) >= 0;
}

// Every thread of a workgroup of THREADS calls this with s[a][threadIdx.x] written: the NA arrays (LDS) become their
// inclusive prefix sums (Hillis-Steele, the arrays side by side between one pair of barriers per step).
template <int THREADS, int NA, class S>
__device__ __forceinline__ void block_scan(S* const (&s)[NA]) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    S add[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) add[a] = t >= off ? s[a][t - off] : (S)0;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NA; ++a) s[a][t] += add[a];
    __syncthreads();
  }
}

// One workgroup of THREADS: items[i * stride], i < n, become their exclusive prefix sums in place; returns their sum.
// Thread t takes a run of consecutive items; the runs' sums (type S) are scanned in s_sum[THREADS].
template <int THREADS, class S>
__device__ __forceinline__ S block_run_scan(uint32_t* items, int64_t n, int64_t stride, S* s_sum) {
  const int64_t per = (n + THREADS - 1) / THREADS;
  const int64_t i0 = (int64_t)threadIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
  S sum = 0;
  for (int64_t i = i0; i < i1; ++i) sum += items[i * stride];
  s_sum[threadIdx.x] = sum;
  S* const runs[1] = {s_sum};
  block_scan<THREADS>(runs);
  S run = s_sum[threadIdx.x] - sum;
  for (int64_t i = i0; i < i1; ++i) {
    const uint32_t c = items[i * stride];
    items[i * stride] = (uint32_t)run;   // (the callers' prefixes are below 2^32)
    run += c;
  }
  return s_sum[THREADS - 1];
}

// The calling wave's part of strip `blockIdx.x`: b[j][e] = the ballot of "row row0 + 256 j + 4 lane + e matches",
// v[j] = the lane's four labels of step j; returns the wave's matches.  row0 (out) = the wave's first row.
__device__ __forceinline__ int strip_ballots(const LabelFilter& f, const uint32_t* s_set, unsigned long long (&b)[LB_ITERS][4],
                                             uint4 (&v)[LB_ITERS], int64_t* row0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * LB_STRIP + (int64_t)wave * LB_WAVE_ROWS;
  *row0 = w0;
  uint32_t dead[LB_ITERS];
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {   // all requested before the first is used
    const int64_t i = w0 + j * 256 + lane * 4;   // a multiple of 4: one 16-byte load, one nibble of a bitmap word
    const bool in = i < f.n;
    v[j] = (f.labels && in) ? ((const uint4*)f.labels)[i >> 2] : make_uint4(0u, 0u, 0u, 0u);
    dead[j] = dead_nibble(in ? f.dead_bits : nullptr, i >> 2);
  }
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {
    const int64_t i = w0 + j * 256 + lane * 4;
    const uint32_t lab[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool hit = i + e < f.n && !((dead[j] >> e) & 1u) && label_in_set(lab[e], f, s_set);
      b[j][e] = __ballot(hit);
      cnt += __popcll(b[j][e]);
    }
  }
  return cnt;
}

__device__ __forceinline__ void strip_stage(const LabelFilter& f, uint32_t* s_set) { label_stage_set(f, s_set); }

// The count pass of a workgroup over its strip, for a FILTER with strip_stage and strip_ballots: counts[blockIdx.x] =
// the strip's matches; *total += them.
template <class FILTER>
__device__ __forceinline__ void strip_count(const FILTER& f, uint32_t* s_set, int* s_wave, uint32_t* __restrict__ counts,
                                            unsigned long long* __restrict__ total) {
  strip_stage(f, s_set);
  unsigned long long b[LB_ITERS][4];
  uint4 v[LB_ITERS];
  int64_t row0;
  const int cnt = strip_ballots(f, s_set, b, v, &row0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < LB_WAVES; ++w) sum += s_wave[w];
    counts[blockIdx.x] = (uint32_t)sum;
    if (sum) atomicAdd(total, (unsigned long long)sum);
  }
}

// The slots of the write pass, from the calling wave's ballots b and their sum cnt: a match's slot is the strip's base +
// the matches in the earlier waves of the strip + the matches before it in its own wave.  put(slot, j, e) is called for
// the lane's own matches -- element e of step j -- whose slot is below m: a slot at or past m is never written.
template <class PUT>
__device__ __forceinline__ void strip_slots(const unsigned long long (&b)[LB_ITERS][4], int cnt, int* s_wave,
                                            const uint32_t* __restrict__ bases, int64_t m, PUT&& put) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = cnt;
  __syncthreads();
  int64_t slot = bases[blockIdx.x];
  for (int w = 0; w < wave; ++w) slot += s_wave[w];   // the matches in the earlier waves of the strip
#pragma unroll
  for (int j = 0; j < LB_ITERS; ++j) {
    // within a step the rows ascend lane by lane, then element by element: the matches of the lanes below, then the
    // lane's own earlier elements
    int below = 0, step = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      below += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b[j][e] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b[j][e], 0u));
      step += __popcll(b[j][e]);
    }
    int64_t s = slot + below;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((b[j][e] >> lane) & 1ull) {
        if (s < m) put(s, j, e);
        ++s;
      }
    }
    slot += step;
  }
}

// Element e of a lane's 16-byte load
__device__ __forceinline__ uint32_t uint4_at(const uint4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// The write pass: the predicate again, then strip_slots.  The payload of a match is its row (LB_ROWS) or the value
// strip_ballots left in v (LB_VALUES: the label filter's).
template <int PAYLOAD, class FILTER>
__device__ __forceinline__ void strip_write(const FILTER& f, uint32_t* s_set, int* s_wave, const uint32_t* __restrict__ bases,
                                            uint32_t* __restrict__ out, int64_t m) {
  strip_stage(f, s_set);
  unsigned long long b[LB_ITERS][4];
  uint4 v[LB_ITERS];
  int64_t row0;
  const int cnt = strip_ballots(f, s_set, b, v, &row0);
  const int lane = threadIdx.x & 63;
  strip_slots(b, cnt, s_wave, bases, m, [&](int64_t s, int j, int e) {
    out[s] = PAYLOAD == LB_ROWS ? (uint32_t)(row0 + j * 256 + lane * 4 + e) : uint4_at(v[j], e);
  });
}

// grid = ceil(n / LB_STRIP) workgroups.  counts[blockIdx.x] = the strip's matches; *total += them (zero on entry).
__global__ __launch_bounds__(LB_THREADS) void label_count_kernel(LabelFilter f, uint32_t* __restrict__ counts,
                                                                 unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ int s_wave[LB_WAVES];
  strip_count(f, s_set, s_wave, counts, total);
}

// One workgroup: counts[0 .. nb) -> their exclusive prefix sums, in place (block_run_scan).
__global__ __launch_bounds__(LB_THREADS) void label_scan_kernel(uint32_t* __restrict__ counts, int64_t nb) {
  __shared__ uint32_t s_sum[LB_THREADS];
  (void)block_run_scan<LB_THREADS>(counts, nb, 1, s_sum);
}

// grid as label_count_kernel, same filter.  bases = the scanned counts; out[0 .. m) receives, in ascending row order,
// the matching rows (PAYLOAD == LB_ROWS: local row indices) or their labels (LB_VALUES).  m = the total the count pass
// found: a slot at or past it is never written.
template <int PAYLOAD>
__global__ __launch_bounds__(LB_THREADS) void label_write_kernel(LabelFilter f, const uint32_t* __restrict__ bases,
                                                                 uint32_t* __restrict__ out, int64_t m) {
  __shared__ uint32_t s_set[LB_MAX_SET];
  __shared__ int s_wave[LB_WAVES];
  strip_write<PAYLOAD>(f, s_set, s_wave, bases, out, m);
}

// pos[0 .. cnt): list positions as run_select wrote them -> out_rows[i] = list[pos[i]] + row_offset; a position
// outside [0, m) -> -1 (the host reports it).
__global__ __launch_bounds__(256) void label_map_rows_kernel(const int64_t* __restrict__ pos, int64_t cnt, const uint32_t* __restrict__ list,
                                                             int64_t m, int64_t row_offset, int64_t* __restrict__ out_rows) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pos[i];
    out_rows[i] = (p >= 0 && p < m) ? (int64_t)list[p] + row_offset : (int64_t)-1;
  }
}

}  // namespace svs

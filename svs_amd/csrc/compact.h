// compact.h -- in-place, order-preserving compaction of the HBM image: every live row moves down over the tombstoned
// ones (svs_index_compact).  Row r goes to dst(r) = r - (dead rows below r), so the result is the matrix a rebuild
// from the live rows would hold, and nothing but a bounce buffer of a few MiB is allocated: a corpus that fills the
// device has no room for a second copy.
//
// Kernel side: one launch moves the rows of a contiguous range of DESTINATIONS [dst0, dst0 + count).  A destination
// p finds its source with a binary search over the ascending device list of dead rows: the smallest j with
// dead[j] - j > p is the number of dead rows at or below the source, src = p + j.  Rows are copied in 16-byte chunks
// (choose_ld: every dtype's row is a whole number of them), by `lanes` lanes per row (a power of two, a wave at
// most), any row length; byte offsets are 64-bit.  An fp8 row takes its f32 scale along, an f32 row with a half
// shadow its shadow row: compile-time forms of the one kernel.  Plain loads and stores.
//
// Hazard and ordering: within one launch a destination may be another live row's source, and workgroups run in any
// order.  Nothing waits inside a launch (no grid-wide spins); the HOST orders the work.  compact_plan cuts
// the destinations [first dead row, n_live) into ascending, contiguous steps, launched in order on one stream:
//   DIRECT(dst0, count)  one launch.  Legal when dst0 + count <= src(dst0): the destination range ends before the
//                        source range begins.  src(dst0) - dst0 is the number of dead rows the sweep has passed, so
//                        the usable count grows as the sweep advances.
//   BOUNCE(dst0, count)  sources -> bounce buffer, then bounce buffer -> destinations: two launches, count <=
//                        bounce_rows.  Taken while the gap is smaller than the bounce buffer.
// Either way a step overwrites only rows that are dead or were moved by an earlier step (a live row r sits at or
// above its destination, so every live row inside [dst0, dst0 + count) has a destination below dst0 + count: it
// went with an earlier step or is read, into the bounce buffer, before this step's first write).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svs {

constexpr int64_t COMPACT_DIRECT = 0, COMPACT_BOUNCE = 1;
constexpr int COMPACT_PLAIN = 0, COMPACT_SCALES = 1, COMPACT_SHADOW = 2;

// Dead rows at or below the source of destination p: the smallest j in [0, ndead] with dead[j] - j > p.
__host__ __device__ inline int64_t compact_dead_below(const uint32_t* dead, int64_t ndead, int64_t p) {
  int64_t lo = 0, hi = ndead;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)dead[mid] - mid > p) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The steps of a compaction (pure host code): steps[3 i ..] = kind, dst0, count, up to cap steps written; returns the
// number of steps the plan has (it may exceed cap), or -1 for a list that is not strictly ascending inside [0, n) or
// a bounce buffer of less than one row.
inline int64_t compact_plan(const uint32_t* dead, int64_t ndead, int64_t n, int64_t bounce_rows, int64_t* steps, int64_t cap) {
  if (ndead < 0 || n < 0 || ndead > n || bounce_rows < 1 || (ndead > 0 && !dead)) return -1;
  for (int64_t j = 0; j < ndead; ++j)
    if ((int64_t)dead[j] >= n || (j > 0 && dead[j] <= dead[j - 1])) return -1;
  if (ndead == 0) return 0;
  const int64_t n_live = n - ndead;
  int64_t nsteps = 0;
  for (int64_t p = dead[0]; p < n_live;) {
    const int64_t gap = compact_dead_below(dead, ndead, p);   // src(p) - p >= 1
    const bool direct = gap >= bounce_rows;
    const int64_t count = (direct ? gap : bounce_rows) < n_live - p ? (direct ? gap : bounce_rows) : n_live - p;
    if (steps && nsteps < cap) {
      steps[3 * nsteps] = direct ? COMPACT_DIRECT : COMPACT_BOUNCE;
      steps[3 * nsteps + 1] = p;
      steps[3 * nsteps + 2] = count;
    }
    ++nsteps;
    p += count;
  }
  return nsteps;
}

// One side of a move: where row t of the launch (destination dst0 + t) lives.  The corpus as a destination and the
// bounce buffer are addressed by t from pointers the host has advanced; the corpus as a source (GATHER) by the
// absolute row dst0 + t + dead rows below, from the buffers' bases.
struct CompactBufs {
  uint4* rows;
  float* scales;    // COMPACT_SCALES
  uint4* shadow;    // COMPACT_SHADOW
};

// A wave takes a batch of 2^batch_log2 <= 64 consecutive destinations at a time (the host picks 64 when the launch
// still fills the device with such batches, fewer for a short step): lane l finds the source of destination l of the
// batch -- up to 64 binary searches side by side cost the latency of one -- then the wave copies the rows, `lanes`
// lanes per row and 64 / lanes rows at a time (a batch holds at least that many), each row's source handed over by a
// shuffle.  Up to four 16-byte chunks per lane are in flight whatever the row length (a 3 KiB row is three chunks
// per lane).
template <int FORM, bool GATHER>
__global__ __launch_bounds__(256) void compact_move_kernel(CompactBufs src, CompactBufs dst, const uint32_t* __restrict__ dead,
                                                           int64_t ndead, int64_t dst0, int64_t count, int chunks, int shadow_chunks,
                                                           int lanes_log2, int batch_log2) {
  const int lanes = 1 << lanes_log2;
  const int wl = (int)(threadIdx.x & 63u);               // lane of the wave
  const int lane = wl & (lanes - 1);                     // lane of the row
  const int sub = wl >> lanes_log2;                      // which of the rows the wave copies at a time
  const int rows_at_a_time = 64 >> lanes_log2;
  const int batch = 1 << batch_log2;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << batch_log2; base < count; base += waves << batch_log2) {
    int64_t s_mine = 0;
    if (GATHER && wl < batch && base + wl < count) s_mine = dst0 + base + wl + compact_dead_below(dead, ndead, dst0 + base + wl);
    for (int r = 0; r < batch && base + r < count; r += rows_at_a_time) {   // (wave-uniform bounds)
      const int64_t s = GATHER ? __shfl(s_mine, r + sub, 64) : base + r + sub;
      const int64_t t = base + r + sub;
      if (t >= count) continue;
      auto copy = [&](const uint4* __restrict__ from, uint4* __restrict__ to, int nch) {
        for (int c = lane; c < nch; c += 4 * lanes) {
          const bool h1 = c + lanes < nch, h2 = c + 2 * lanes < nch, h3 = c + 3 * lanes < nch;
          const uint4 a0 = from[c];
          uint4 a1 = a0, a2 = a0, a3 = a0;
          if (h1) a1 = from[c + lanes];
          if (h2) a2 = from[c + 2 * lanes];
          if (h3) a3 = from[c + 3 * lanes];
          to[c] = a0;
          if (h1) to[c + lanes] = a1;
          if (h2) to[c + 2 * lanes] = a2;
          if (h3) to[c + 3 * lanes] = a3;
        }
      };
      copy(src.rows + (size_t)s * (size_t)chunks, dst.rows + (size_t)t * (size_t)chunks, chunks);
      if constexpr (FORM == COMPACT_SHADOW)
        copy(src.shadow + (size_t)s * (size_t)shadow_chunks, dst.shadow + (size_t)t * (size_t)shadow_chunks, shadow_chunks);
      if constexpr (FORM == COMPACT_SCALES)
        if (lane == 0) dst.scales[t] = src.scales[s];
    }
  }
}

}  // namespace svs

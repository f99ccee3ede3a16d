// Shared corpus passes of the run-ahead pipeline (svs_index_search_device_ahead; DESIGN.md 4, "Shared passes").
//
// Single-query searches queued on one pipeline all stream the same half rows.  When pass i starts, the queries of the
// searches i+1, i+2, ... are usually complete in device memory already, so pass i serves them from the row registers
// it has just loaded (gemv_f16_oneshot_kernel with a PassPlan): no HBM byte more, and every score keeps the arithmetic
// of a pass of its own.  The later searches' own passes then find nothing to do and return before their first load.
//
// What a pass serves is decided in ONE place, pass_claim_kernel: one workgroup on the pass stream directly in front of
// the pass.  All workgroups of the pass read that one decision across the kernel boundary; none of them reads memory
// the host may still be writing, nothing spins or polls, and the pass grid issues no atomics.
//
// Thin grids.  A search that an earlier pass serves still launches its own pass, which returns at c == 0; the host
// cannot know what the claim kernel will decide, but it can almost always guess (enqueue_ahead keeps its own copy of the
// rule below) and then launches that pass on one resident set of workgroups instead of the one-shot grid.  The guess
// is a hint: the kernel walks all row blocks on any grid, so a thin pass that does have work computes the same scores,
// only slower.  The claim kernel counts the thin passes and those among them that had work.
//
// Publication: every shareable call writes its search into the pipeline's mailbox (pinned host memory, indexed by the
// search number modulo MAILBOX_SIZE) before it launches anything: tag 0, the fields, then tag = number + 1 with
// release ordering.  The claim kernel reads tag, fields, tag with system-scope loads and takes an entry only when both
// tags are the expected one; an entry the host has overwritten (it ran more than a mailbox ahead) or is still writing
// is simply not claimed, and that search is served by its own pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemv_f32.h"

namespace svs {

constexpr int SHARE_MAX = 4;           // queries one pass can serve (compile-time bound of the plan)
constexpr int SHARE_DEFAULT = 4;       // ... and what a pipeline's passes serve unless svs_internal_tune(5, v) says otherwise
constexpr int MAILBOX_SIZE = 1024;     // entries per pipeline (power of two)
static_assert(SHARE_MAX >= 1 && SHARE_MAX <= 4, "the plan and the claim kernel's gather are laid out for at most 4");
static_assert((MAILBOX_SIZE & (MAILBOX_SIZE - 1)) == 0 && MAILBOX_SIZE >= 1024, "mailbox: a power of two, >= 1024 entries");

// What the pass in front of which it was written serves: c queries (0: nothing), each with its score vector.
struct PassPlan {
  uint32_t c;
  uint32_t pad;
  const v4f* q[SHARE_MAX];
  float* scores[SHARE_MAX];
};

constexpr uint32_t MAIL_CLAIMABLE = 1u;   // MailEntry::flags: an earlier pass may serve this search

// One published search: 8 x 8 bytes, so that eight lanes fetch an entry in one wave-wide load.
struct MailEntry {
  uint64_t tag;      // search number + 1 (0: being written)
  uint64_t q;        // the query as the pass reads it: ld floats, 16-byte aligned
  uint64_t scores;   // the score vector of the search's context
  uint64_t rows;     // the half rows its pass reads ...
  uint64_t n;        // ... how many ...
  uint64_t epoch;    // ... and the index's geometry epoch at the call
  uint64_t ld;       // row length (halves)
  uint64_t flags;
};
static_assert(sizeof(MailEntry) == 64, "claim kernel: eight 8-byte words per entry");
constexpr int SHARE_MIRROR_WORDS = SHARE_MAX + 1 + 2;   // pinned mirror of ShareState::hist and ::thin, in that order

// Device-side state of one pipeline, touched by its claim kernels only (stream order: one at a time).
struct ShareState {
  uint64_t served;                 // every search of the pipeline with a number below this has been served by a pass
  uint32_t hist[SHARE_MAX + 1];    // passes that served 0 (empty), 1, 2, ... queries
  uint32_t thin[2];                // passes launched on a thin grid; those among them that served c > 0 queries
  PassPlan plan;                   // of the pass behind the claim kernel that ran last
};

// Search `num` is about to run its pass (q, scores: its own; rows / n / epoch / ld: what the pass reads).  `reach`:
// the last search whose context the waits already enqueued in front of this pass let it write.  `limit`: queries the
// pass may serve (<= SHARE_MAX).  mirror: SHARE_MIRROR_WORDS words of pinned memory that follow st->hist and st->thin
// (plain stores, as the re-score kernel's counters).  thin: the pass behind this kernel is launched on a thin grid.
__global__ __launch_bounds__(64) void pass_claim_kernel(const MailEntry* mailbox, ShareState* st, uint32_t* mirror,
                                                        uint64_t num, uint64_t reach, int limit, const v4f* q,
                                                        float* scores, uint64_t rows, uint64_t n, uint64_t epoch,
                                                        uint64_t ld, int thin) {
  __shared__ uint64_t ent[SHARE_MAX][8];
  const int lane = threadIdx.x;
  const bool served = st->served > num;   // (uniform: an earlier pass took this search)
  const int want = served ? 0 : (limit < SHARE_MAX ? limit : SHARE_MAX) - 1;   // successors to look at
  const int e = lane >> 3, w = lane & 7;
  if (e < want) {
    const uint64_t* p = (const uint64_t*)&mailbox[(num + 1 + e) & (MAILBOX_SIZE - 1)];
    const uint64_t t0 = __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint64_t v = w == 0 ? t0 : __hip_atomic_load(p + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const uint64_t t1 = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // (every lane brackets its own word with the two tag reads; a word that was not read under this search's tag is
    //  0, which none of the checks below accepts: epochs start at 1, pointers, n and ld are never 0)
    ent[e][w] = t0 == t1 && t0 == num + 2 + e ? v : 0;
  }
  __syncthreads();
  if (lane != 0) return;
  PassPlan plan{};
  if (!served) {
    plan.q[0] = q;
    plan.scores[0] = scores;
    int c = 1;
    for (int k = 0; k < want; ++k) {
      const uint64_t s = num + 1 + k;
      bool ok = s <= reach && ent[k][0] == s + 1;
      ok = ok && (ent[k][7] & MAIL_CLAIMABLE) && ent[k][3] == rows && ent[k][4] == n && ent[k][5] == epoch && ent[k][6] == ld &&
           ent[k][1] != 0 && ent[k][2] != 0;
      if (!ok) break;
      plan.q[c] = (const v4f*)ent[k][1];
      plan.scores[c] = (float*)ent[k][2];
      ++c;
    }
    plan.c = (uint32_t)c;
    st->served = num + c;
  }
  st->plan = plan;
  const uint32_t h = st->hist[plan.c] + 1u;
  st->hist[plan.c] = h;
  mirror[plan.c] = h;
  if (thin) {
    const int w = plan.c ? 1 : 0;   // (a thin pass with work: the host's guess was wrong, the pass strides over the corpus)
    const uint32_t t = st->thin[0] + 1u;
    st->thin[0] = t;
    mirror[SHARE_MAX + 1] = t;
    if (w) {
      const uint32_t tw = st->thin[1] + 1u;
      st->thin[1] = tw;
      mirror[SHARE_MAX + 2] = tw;
    }
  }
}

}  // namespace svs

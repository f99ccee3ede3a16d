// C ABI of the MI355X similarity backend (see include/svs_amd.h).
// Host side: HBM-resident corpus handle, per-call search contexts (stream +
// scratch, so searches are re-entrant), launch sequencing of the score stage
// (gemv_f32.h) and the top-k stage (select.h).  gfx950 only.
#include "../../include/svs_amd.h"
#include "coalesce.h"
#include "internal.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <mutex>
#include <shared_mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "fp8.h"
#include "gather.h"
#include "gemm_tiled.h"
#include "gemm_phased.h"
#include "gemm_q16.h"
#include "gemv_unrolled.h"
#include "gemv_f16.h"
#include "gemv_f32.h"
#include "select.h"
#include "screen.h"
#include "compact.h"
#include "neighbors.h"
#include "segments.h"
#include "above.h"
#include "combine.h"
#include "diverse.h"
#include "labels.h"
#include "where.h"
#include "by_label.h"
#include "collapse.h"
#include "collapse_combine.h"
#include "collapse_scope.h"
#include "assign.h"
#include "label_sums.h"

namespace {

using namespace svs;

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(e_ == hipErrorOutOfMemory ? SVS_ERR_NOMEM : SVS_ERR_DEVICE, "%s: %s (%s:%d)", \
                  #expr, hipGetErrorString(e_), __FILE__, __LINE__);                        \
  } while (0)

// Scratch that frees itself: pointer + capacity (in elements), device memory or pinned host memory.  grow(need) does
// nothing when `need` fits; otherwise it frees, then allocates: the old contents are NOT kept, and the capacity is 0
// after a failed allocation.
template <typename T, bool PINNED>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { (void)release(); }
  operator T*() const { return p; }
  hipError_t release() {
    hipError_t e = hipSuccess;
    if (p) e = PINNED ? hipHostFree(p) : hipFree(p);
    p = nullptr;
    cap = 0;
    return e;
  }
  int grow(size_t need) {
    if (need <= cap) return SVS_OK;
    HIP_TRY(release());
    if constexpr (PINNED) HIP_TRY(hipHostMalloc((void**)&p, need * sizeof(T), hipHostMallocDefault));
    else HIP_TRY(hipMalloc((void**)&p, need * sizeof(T)));
    cap = need;
    return SVS_OK;
  }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

// ---- internal tunables (svs_internal_tune: tools and tests; not part of the ABI) --------------------
std::atomic<int64_t> g_tune_prefix_div{64};   // fused path: rows of the threshold prefix = n / this (>= FUSE_PREFIX_MIN)
std::atomic<int64_t> g_tune_upload{0};        // host batches: 0 = f16 batches are PULLED from pinned memory by the staging kernel, chunk by chunk
                                              // (no DMA, no f32 copy in HBM); 1 = round 3's staging + DMA for every dtype
std::atomic<int64_t> g_tune_spread{1};        // fused path: 1 = thresholds from a sample spread over the whole corpus (prefix_image), 0 = from its first rows (rounds 1-3)
std::atomic<int64_t> g_tune_refuse_shadow{0}; // 1 = every allocation of an f32 index's half shadow "fails" (tests of the best-effort path)
std::atomic<int64_t> g_tune_handover{0};      // run-ahead pipelines made from now on: 0 = the pass carries its completion event and the pass stream
                                              // waits once per group of passes; 1 = a record and a wait per pass
std::atomic<int64_t> g_tune_share{SHARE_DEFAULT};  // run-ahead pipelines made from now on: queries one score pass may serve (1: its own search only)
std::atomic<int64_t> g_tune_thin{0};          // run-ahead pipelines, grid of a shareable search's pass: 0 = thin where the host predicts that an earlier pass
                                              // serves the search, 1 = always the one-shot grid, 2 = always thin (tests)
std::atomic<int64_t> g_tune_by_label_cross{BL_ATOMIC};  // svs_index_search_by_label, what crosses workgroups: BL_ATOMIC = integer atomics on the query's
                                              // table in HBM, BL_PARTIALS = a partial table per workgroup, reduced by the final kernel (the same bits)
std::atomic<int64_t> g_tune_combine_route{0};  // svs_index_search_combined: 0 = the route's choice (combine_route), 1 = fused wherever a fused kernel
                                              // exists, 2 = always m passes (tools/combined_time.py)
thread_local double g_host_phase[6];         // svs_internal_host_phases: seconds since the call began (last svs_index_search on this thread)

// svs_internal_last_launches: the score kernels the calling thread's last search / scores call enqueued, in order: every
// batched launch (launch_batched), and for the single-query kernels a "gemv" entry per loop (launch_batch,
// svs_index_scores_n) followed by the kernel of each query (launch_single).  Fixed thread-local slots and names that are compile-time
// constants: recording is a few stores, no allocation, no lock; entries past LAUNCH_REC_CAP are dropped.
struct LaunchRec {
  const char* kernel;
  int64_t rows;
  int32_t nq;
};
constexpr int LAUNCH_REC_CAP = 64;   // (svs_index_top_pairs over 17 k rows: 17 prefix + 17 pair-mode launches)
thread_local LaunchRec g_launch[LAUNCH_REC_CAP];
thread_local int32_t g_nlaunch;                // launches since the reset (may exceed LAUNCH_REC_CAP: those are not kept)

inline void launch_reset() { g_nlaunch = 0; }
inline void launch_record(const char* kernel, int64_t rows, int nq) {
  if (g_nlaunch < LAUNCH_REC_CAP) g_launch[g_nlaunch] = LaunchRec{kernel, rows, (int32_t)nq};
  ++g_nlaunch;
}

// "name<a, b, ...>": a kernel and its template arguments spelled as c++filt prints them (the build's resource report),
// built at compile time
struct KernelName {
  char s[64] = {};
};
template <class... A>
constexpr KernelName kernel_name(const char* base, A... args) {
  KernelName k{};
  int p = 0;
  for (const char* c = base; *c; ++c) k.s[p++] = *c;
  k.s[p++] = '<';
  int i = 0;
  auto put = [&](auto v) {
    if (i++) { k.s[p++] = ','; k.s[p++] = ' '; }
    if constexpr (std::is_same_v<decltype(v), bool>) {
      for (const char* c = v ? "true" : "false"; *c; ++c) k.s[p++] = *c;
    } else if constexpr (std::is_same_v<decltype(v), const char*>) {   // a type argument, spelled by the caller
      for (const char* c = v; *c; ++c) k.s[p++] = *c;
    } else {
      long long x = v;
      if (x < 0) { k.s[p++] = '-'; x = -x; }
      char dig[20] = {};
      int nd = 0;
      do { dig[nd++] = (char)('0' + x % 10); x /= 10; } while (x);
      while (nd) k.s[p++] = dig[--nd];
    }
  };
  (put(args), ...);
  k.s[p++] = '>';
  return k;
}

// What a single-query score launch is given besides its operands: enqueue_score_half -> launch_scores -> the launcher.
struct PassOpts {
  hipEvent_t stop = nullptr;       // the completion event of the score half, when this is its LAST kernel (launch_tail)
  const PassPlan* plan = nullptr;  // f16 one-shot kernel of a geometry that shares: the plan the pass serves (pass_share.h),
  int limit = 0;                   // ... the most queries it may hold (the launch's dynamic LDS),
  bool thin = false;               // ... and the pass on one resident set of workgroups instead of the one-shot grid
  const char** name = nullptr;     // svs_internal_single_route: launch nothing, store the kernel's name here
};
// stop: the completion event of a score half, carried by this launch (an extended launch) instead of a record behind it
template <class... P, class... A>
inline void launch_tail(hipEvent_t stop, void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t st, A&&... args) {
  if (stop) hipExtLaunchKernelGGL<P...>(kernel, grid, block, lds, st, nullptr, stop, 0, static_cast<P>(args)...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
}
// Every single-query score launch: recorded and launched, or (o.name) named only
template <class... P, class... A>
inline void launch_single(const PassOpts& o, const char* name, int64_t rows, void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds,
                          hipStream_t st, A&&... args) {
  if (o.name) { *o.name = name; return; }
  launch_record(name, rows, 1);
  launch_tail(o.stop, kernel, grid, block, lds, st, static_cast<A&&>(args)...);
}
// Every batched score launch (gemm_q16.h, gemm_tiled.h, gemm_phased.h): named only (name_only, svs_internal_batch_route:
// before anything here touches HIP), or recorded and launched -- the first launch of a kernel raises its dynamic-LDS
// limit to lds_max
template <auto Kernel, class... A>
inline void launch_batched(const char** name_only, const char* name, int lds_max, int64_t rows, int nq, dim3 grid, dim3 block, size_t lds,
                           hipStream_t st, A... args) {
  if (name_only) { *name_only = name; return; }
  static std::once_flag once;
  std::call_once(once, [&] { (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max); });
  launch_record(name, rows, nq);
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
}

struct EvTriple {
  hipEvent_t e0, e1, e2;
  hipEvent_t d0 = nullptr, d1 = nullptr;   // around the dominant kernel of a fused search (else unset)
};
void ev_destroy(EvTriple& t) {
  (void)hipEventDestroy(t.e0);
  (void)hipEventDestroy(t.e1);
  (void)hipEventDestroy(t.e2);
  if (t.d0) (void)hipEventDestroy(t.d0);
  if (t.d1) (void)hipEventDestroy(t.d1);
}

// One in-flight search: stream, device scratch, pinned staging.
struct Ctx {
  hipStream_t stream = nullptr;
  DevBuf<float> q_dev;
  DevBuf<float> q16;            // [16][ld] zero-padded query group
  DevBuf<_Float16> qh;          // half queries, [rows][ld] zero padded
  DevBuf<uint8_t> q8;           // e4m3 queries [rows][ld], zero padded
  DevBuf<float> q8f;            // the same values as f32 (single-query kernel)
  DevBuf<float> q8s;            // query scales
  DevBuf<float> pref_s;         // fused GEMM: top-k of the prefix rows (thresholds)
  DevBuf<int64_t> pref_r;
  DevBuf<float> scores;
  DevBuf<uint32_t> hist;        // histogram and candidate counters, then the candidate lists: one capacity, allocated,
  DevBuf<uint64_t> cand;        // zeroed and released together (grow_select_scratch)
  size_t hist_cap = 0;          // queries
  DevBuf<uint64_t> keys;
  PinBuf<float> q_pin;
  PinBuf<float> out_s_pin;      PinBuf<int64_t> out_r_pin;
  PinBuf<float> redo_s_pin;     PinBuf<int64_t> redo_r_pin;   // results of re-run queries (search_host)
  PinBuf<float> redo_q_pin;                                    // ... and the queries themselves, gathered
  DevBuf<uint32_t> list_dev;    // svs_index_search_rows: the listed local rows (u32)
  PinBuf<uint32_t> list_pin;    // ... built here, uploaded from here
  // svs_index_neighbors (neighbors.h): the call's local source rows (pinned copy, device copy), the block's search
  // results at stride count + 1, and the re-run groups' row lists and query panel
  PinBuf<uint32_t> nb_list_pin; DevBuf<uint32_t> nb_list_dev;
  DevBuf<float> nb_s;           DevBuf<int64_t> nb_r;
  PinBuf<uint32_t> nb_redo_pin; DevBuf<uint32_t> nb_redo_dev;
  DevBuf<float> nb_redo_q;
  // svs_index_search_segments (segments.h): the tile table followed by the small segments' table (16-byte entries,
  // pinned copy and device copy), and the result block -- int64 rows, then f32 scores -- that comes back in one copy
  PinBuf<SegTile> seg_plan_pin; DevBuf<SegTile> seg_plan_dev;
  DevBuf<int64_t> seg_res_dev;  PinBuf<int64_t> seg_res_pin;
  // svs_index_search_above (above.h): per query, the entries the device wrote (-1: re-run on the host) and the total
  PinBuf<int32_t> above_cnt_pin; PinBuf<int64_t> above_tot_pin;
  // svs_index_search_diverse (diverse.h): a block of queries' c x c similarity matrices (at most DIVERSE_G_BUDGET bytes)
  // and the call's picks; the candidates are read where the search left them, in out_s_pin / out_r_pin
  DevBuf<float> dv_G;
  PinBuf<float> dv_s_pin;       PinBuf<int64_t> dv_r_pin;     PinBuf<float> dv_red_pin;
  // The call's labels, pinned and device copy: a sorted set (LabelSet::stage) or svs_index_assign's vector labels
  PinBuf<uint32_t> lab_set_pin; DevBuf<uint32_t> lab_set_dev;
  // svs_index_search_labeled (labels.h): the call's total (one u64) followed by the per-strip counts, which the scan
  // turns into the strips' bases; the total's pinned copy; and the list positions the top-k stage writes, mapped to
  // rows on the device.  The list itself is list_dev.
  DevBuf<uint32_t> lab_cnt;     PinBuf<unsigned long long> lab_tot_pin;
  DevBuf<int64_t> lab_pos;
  // svs_index_search_by_label (by_label.h): the query's table of BL_TAB_WORDS words, zeroed when allocated and left
  // zeroed by the final kernel; the workgroups' partial tables (svs_internal_tune(7, 1) only); per query the labels and
  // totals the device wrote (scores and rows: out_s_pin / out_r_pin), then nq counts followed by nq group counts.
  DevBuf<unsigned long long> bl_tab;
  DevBuf<unsigned long long> bl_part_best; DevBuf<uint32_t> bl_part_cnt;
  PinBuf<uint32_t> bl_lab_pin;  PinBuf<int64_t> bl_tot_pin;   PinBuf<int32_t> bl_cnt_pin;
  // svs_index_search_collapsed (collapse.h): the open-addressing table (CL_SLOT_WORDS words per slot), grown to the row
  // count, EMPTY (all zero) between queries and between calls -- cl_clean is false from a query's first insert until
  // the fill behind its mark kernel is enqueued, so a call that left early is repaired by the next one; the queries'
  // survivor counters and their pinned copy; the values of the returned rows (scores and rows: out_s_pin / out_r_pin).
  // All four collapse entries use them through CollapseFrame, the only writer of cl_clean and cc_clean.
  DevBuf<unsigned long long> cl_tab;
  bool cl_clean = true;
  DevBuf<unsigned long long> cl_cnt; PinBuf<unsigned long long> cl_cnt_pin;
  PinBuf<uint32_t> cl_val_pin;
  // svs_index_search_collapsed_combined (collapse_combine.h): beside cl_tab, m per-vector keys for every slot, EMPTY
  // (all zero) between queries and between calls under a flag of its own -- the entries without keys repair only cl_tab
  DevBuf<uint32_t> cc_keys;
  bool cc_clean = true;
  // svs_index_search_collapsed_where / _rows (collapse_scope.h): the group column compacted beside list_dev, padded to
  // whole groups of four.  The table, cl_clean, the counters and the values' pinned copy are the unscoped entry's.
  DevBuf<uint32_t> sc_vals;
  // svs_index_assign (assign.h): the call's vectors in the index's storage format (rows of ld elements; fp8: their
  // scales), the per-row results and the counts.  The f32 vectors go up through q_pin / q_dev.
  DevBuf<uint8_t> as_vec;       DevBuf<float> as_vec_scales;
  DevBuf<int32_t> as_best;      DevBuf<float> as_score;
  DevBuf<unsigned long long> as_cnt;
  // svs_index_label_sums (label_sums.h): the call's row_labels on the device; the strips' histogram; per slot the
  // label's rows, its first list position and its first chunk (3 LB_MAX_SET + 1 words); the label-major row list; the
  // chunk table; the chunks' partial sums; the (nset, d) image of the sums and its pinned copy; the counts' pinned copy.
  DevBuf<uint32_t> ls_lab;      DevBuf<uint32_t> ls_hist;
  DevBuf<unsigned long long> ls_tot;
  DevBuf<uint32_t> ls_list;     DevBuf<LsChunk> ls_table;
  DevBuf<double> ls_part;       DevBuf<double> ls_out;
  PinBuf<double> ls_out_pin;    PinBuf<unsigned long long> ls_cnt_pin;
  // Scratch is reused in stream order.  A context stays with the stream that
  // last used it; handing it to ANOTHER stream first drains the old one.
  hipStream_t last_stream = nullptr;
  bool async_pending = false;
  int slot = 0;                 // this context's counters in svs_index::scr_dev / scr_host (screened search)
};

// svs_index_search_device_ahead: the ordered pipeline of one (index, caller stream).  Score passes run one after
// another on `pass`; search i uses ctx[i % AHEAD_RING], and its selection chain runs on the caller's stream behind
// pass_done, beside the passes of the searches after it.  The contexts never enter svs_index::free_ctx and own no
// stream.  A pass may overwrite the scratch of search s's context once selection s - AHEAD_RING is over.  The caller's
// stream is in order -- a selection that is over means every earlier one is -- so the pass stream does not wait in
// front of every pass but once per AHEAD_GROUP passes: at the passes with i % AHEAD_GROUP == 0 (i >= AHEAD_LAG), for
// the selection of search i - AHEAD_LAG.  Behind that wait every selection up to i - AHEAD_LAG is over, so the
// contexts of the searches up to i - AHEAD_LAG + AHEAD_RING may be written: that is the `reach` of the passes
// i .. i + AHEAD_GROUP - 1 (AheadPipe::covered; a wait a LATER call enqueues cannot protect an earlier pass).  A pass
// serves its own search and up to SHARE_MAX - 1 searches behind it (pass_share.h), so the last pass of a group,
// i + AHEAD_GROUP - 1, reaches SHARE_MAX searches when
//     i - AHEAD_LAG + AHEAD_RING >= i + AHEAD_GROUP - 1 + SHARE_MAX - 1.
// The lag is kept as large as that allows: the older the selection a pass waits for, the less likely it is still
// running.  (A pipeline made under svs_internal_tune(4, 1) waits in front of EVERY pass from the AHEAD_LAG-th on.)
constexpr int AHEAD_RING = 8;
constexpr int AHEAD_GROUP = 2;
constexpr int AHEAD_LAG = 4;
static_assert(AHEAD_LAG >= 1 && AHEAD_GROUP >= 1 && AHEAD_LAG <= AHEAD_RING - AHEAD_GROUP - SHARE_MAX + 2,
              "the wait rule above: every pass of a group must reach SHARE_MAX searches");
static_assert(AHEAD_LAG + AHEAD_GROUP - 1 <= AHEAD_RING, "a pass's own context must be covered by its group's wait");
struct AheadPipe {
  std::mutex mu;                               // one ahead call at a time per pipeline
  hipStream_t caller = nullptr;                // the key
  hipStream_t pass = nullptr;
  Ctx* ctx[AHEAD_RING] = {};
  hipEvent_t pass_done[AHEAD_RING] = {};       // the end of the score half of the context's last search (carried by its last kernel, or recorded on `pass`)
  hipEvent_t sel_done[AHEAD_RING] = {};        // on the caller's stream, behind its selection half: the last reader of the scratch
  bool used[AHEAD_RING] = {};
  bool per_pass = false;                       // svs_internal_tune(4, 1) when the pipeline was made: a record and a wait per pass
  uint64_t seq = 0;                            // searches since the pipeline last drained (0: every context is free)
  uint64_t covered = 0;                        // selections of the searches seq < covered are over for everything enqueued on `pass` from now on
  // shared passes (pass_share.h).  Search numbers never start over: number = base + seq.
  uint64_t base = 0;
  int share_limit = 1;                         // svs_internal_tune(5, v) when the pipeline was made
  MailEntry* mailbox = nullptr;                // pinned: MAILBOX_SIZE entries, then the mirror of ShareState::hist and ::thin
  ShareState* share_dev = nullptr;
  uint32_t* share_mirror() const { return (uint32_t*)(mailbox + MAILBOX_SIZE); }
  // The host's copy of the claim rule (enqueue_ahead: which searches get a thin grid).  A hint only: it may disagree
  // with the device after a wrong guess, until the next search nothing can claim or the next drain.
  struct Owner {
    bool valid = false;                        // the last shareable search the host took for served by its own pass ...
    uint64_t num = 0, next = 0, reach = 0;     // ... its number, the first search behind its run, its reach,
    uint64_t rows = 0, n = 0, epoch = 0, ld = 0;   // what its pass reads,
    uint32_t ordinal = 0;                      // and which claim kernel of the pipeline is its own (counted as `claims`)
  } owner;
  uint32_t claims = 0;                         // claim kernels enqueued so far; those that have run: the sum of the mirrored hist
  uint32_t claims_run() const {
    const volatile uint32_t* h = share_mirror();
    uint32_t s = 0;
    for (int c = 0; c <= SHARE_MAX; ++c) s += h[c];
    return s;
  }
  uint64_t tick = 0;                           // svs_index::pipe_tick of the last call that looked it up (under svs_index::mu)
};

}  // namespace

struct svs_index {
  std::atomic<int> refs{1};
  int device = 0;
  int64_t n = 0;
  int d = 0, ld = 0, dtype = SVS_DTYPE_F32;
  int64_t row_offset = 0;
  int64_t cap = 0;               // rows the buffers can hold (append grows them)
  void* rows = nullptr;
  float* row_scales = nullptr;   // fp8 only: one f32 per row
  size_t bytes = 0;
  // svs_index_set_labels: one u32 per row of the CAPACITY (rounded up to 4: the kernels load 16 bytes), HBM only; null
  // until the first call -- every label is then 0.  Invariant: the labels of the rows from n on are 0, so that rows
  // appended later carry label 0 without a write.  Written under the exclusive geometry lock, read under the shared one.
  // svs_index_set_column: cols[0] IS that label column; columns 1 .. SVS_COLUMNS_MAX - 1 follow the same rules, each
  // null until its own first write.  An allocated column has label_column_bytes(cap) bytes.
  uint32_t* cols[SVS_COLUMNS_MAX] = {};
  size_t col_bytes[SVS_COLUMNS_MAX] = {};
  size_t cols_bytes() const { size_t b = 0; for (size_t cb : col_bytes) b += cb; return b; }
  // Corpus geometry lock: searches hold it shared while they enqueue (and, for the
  // host API, until their results are back); append / mask_rows take it exclusive.
  std::shared_mutex rw;
  std::vector<uint8_t> dead_flag;      // host, one per row
  std::vector<uint32_t> dead_list;     // host copy of the masked (tombstoned) local rows
  DevBuf<uint32_t> dead_dev;           // device copy
  std::vector<uint32_t> dead_bits;     // host bitmap, one bit per row (bit r & 31 of word r >> 5)
  DevBuf<uint32_t> dead_bits_dev;      // device copy (capacity in words): the fused top-k path drops masked candidates with it
  int cu_count = 256;
  // The fused batch path's threshold sample ("prefix image", prefix_image()): pfx_nmat rows copied out of the corpus in
  // blocks of PFX_BLOCK rows taken every pfx_stride rows, as one contiguous matrix the batched kernels can run over.
  // Valid while pfx_n == n (an append / reserve / staging commit moves or extends the rows: they reset pfx_n).
  void* pfx_rows = nullptr;
  float* pfx_scales = nullptr;
  size_t pfx_cap = 0;                  // rows the two buffers hold
  int64_t pfx_n = -1, pfx_nmat = 0, pfx_stride = 0;
  const void* pfx_src = nullptr;       // idx->rows when the image was taken (a reallocation moves the rows)
  std::mutex pfx_mu;

  // Screened single-query search (screen.h): an IEEE-half shadow of an f32 corpus, same capacity and row stride (in
  // elements) as `rows`, kept in step by every ingest path under the locks those paths hold.  Best effort: an
  // allocation that fails drops the shadow and the index searches unscreened.
  void* shadow = nullptr;
  size_t shadow_bytes = 0;
  uint32_t* scr_dev = nullptr;         // ScreenStats, then kSlots x SCREEN_SLOT_WORDS per-context counters
  uint32_t* scr_host = nullptr;        // pinned mirror of the counters, written by the kernels
  std::atomic<bool> shadow_bad{false}; // an element that half cannot hold: never screens again
  bool shadow_gave_up = false;         // an allocation failed: not retried until svs_index_set_screen(1)
  bool stats_dirty = false;            // a staging commit's conversion is still queued (under stg_mu)
  std::atomic<int> screen_mode{1};     // svs_index_set_screen
  std::atomic<bool> scr_paused{false}; // fallbacks dominated recent queries: no screening until the next ingest
  std::atomic<uint64_t> scr_base_s{0}, scr_base_f{0};
  // Bumped by everything that changes n, the row pointers, the shadow or the score route (under the exclusive
  // geometry lock, or where a search drops the screen): a shared pass never serves a search planned under another one.
  std::atomic<uint64_t> geo_epoch{1};

  std::mutex mu;
  std::condition_variable cv;
  std::vector<Ctx*> free_ctx;
  int n_ctx = 0;
  static constexpr int kMaxCtx = 8;
  // svs_index_search_device_ahead: one pipeline per caller stream (guarded by mu), at most kMaxPipes of them; they
  // live until the index goes.  A stream that has none when all exist takes over the least recently used pipeline
  // that is IDLE (pipe_get); only when every pipeline has work in flight is the call a plain one, and counted.
  // Counter slots: the pooled contexts take [0, kMaxCtx), pipeline p's contexts the AHEAD_RING slots from
  // kMaxCtx + AHEAD_RING p on.
  static constexpr int kMaxPipes = 4;
  static constexpr int kSlots = kMaxCtx + AHEAD_RING * kMaxPipes;
  std::vector<AheadPipe*> pipes;
  uint64_t pipe_tick = 0;
  std::atomic<int64_t> ahead_calls{0}, ahead_plain{0}, ahead_retired{0};   // svs_internal_ahead_stats
  std::atomic<int64_t> ahead_bound{0}, ahead_records{0}, ahead_waits{0};   // ... what the calls put on their pass streams

  // cold-start staging (svs_index_staging_*): two pinned blocks, DMA'd on their own stream
  struct Staging {
    void* pin[2] = {nullptr, nullptr};
    float* dstage[2] = {nullptr, nullptr};   // f16 / fp8: the f32 block lands here, a kernel converts it
    hipEvent_t done[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    int cur = 1;                             // block handed out by the last acquire
    int64_t rows_cap = 0;
    bool active = false;
  } stg;
  std::mutex stg_mu;
  std::atomic<bool> staging_pending{false};

  // svs_index_set_coalesce: single-query host searches that are in flight together share corpus passes
  std::atomic<bool> coalesce{false};
  std::atomic<bool> co_round{true};
  svs::Coalescer co;

  std::atomic<int> timing{0};          // 0 off, N: time every N-th search
  std::atomic<uint32_t> timing_seq{0};
  std::atomic<int> variant{0};
  std::vector<EvTriple> evs;  // guarded by mu
};

namespace {

// Floats from one score vector of n rows to the next: float4-aligned, as the select and strip kernels load them
constexpr int64_t score_stride(int64_t n) { return (n + 3) & ~(int64_t)3; }

// The device's dead-row bitmap (dead_bits.h), null while no row is masked
inline const uint32_t* dead_bits_of(const svs_index* idx) { return idx->dead_list.empty() ? nullptr : idx->dead_bits_dev.p; }

void ctx_destroy(Ctx* c) {
  if (!c) return;
  if (c->async_pending) (void)hipStreamSynchronize(c->last_stream);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  hipStream_t st = c->stream;
  delete c;   // (frees every buffer)
  if (st) (void)hipStreamDestroy(st);
}

// Everything the pipeline has enqueued is over: its passes, and the selection chains on the caller's stream.  The
// chains are waited for through the pipeline's OWN events (the caller may have destroyed its stream since; an event
// that was never recorded counts as fired).
// Afterwards the ring starts over (seq = 0): no context is in use, and the next AHEAD_RING passes wait for nothing.
hipError_t pipe_drain(AheadPipe* p) {
  hipError_t e = hipStreamSynchronize(p->pass);
  for (int j = 0; j < AHEAD_RING; ++j) {
    const hipError_t e2 = p->sel_done[j] ? hipEventSynchronize(p->sel_done[j]) : hipSuccess;
    if (e == hipSuccess) e = e2;
    p->used[j] = false;
  }
  p->base += p->seq;   // (search numbers go on: a pass that has run never meets a later search under its number)
  p->owner.valid = false;
  if (p->mailbox) p->claims = p->claims_run();   // (every claim kernel has run; one whose launch failed never will)
  p->seq = 0;
  p->covered = 0;
  return e;
}

void pipe_destroy(AheadPipe* p) {
  if (!p) return;
  if (p->pass) (void)pipe_drain(p);
  for (int j = 0; j < AHEAD_RING; ++j) {
    ctx_destroy(p->ctx[j]);   // (drained above; the contexts own no stream)
    if (p->pass_done[j]) (void)hipEventDestroy(p->pass_done[j]);
    if (p->sel_done[j]) (void)hipEventDestroy(p->sel_done[j]);
  }
  if (p->pass) (void)hipStreamDestroy(p->pass);
  if (p->mailbox) (void)hipHostFree(p->mailbox);
  (void)hipFree(p->share_dev);
  delete p;
}

void staging_free(svs_index* idx) {
  auto& g = idx->stg;
  if (g.st) (void)hipStreamSynchronize(g.st);
  for (int i = 0; i < 2; ++i) {
    if (g.pin[i]) (void)hipHostFree(g.pin[i]);
    if (g.dstage[i]) (void)hipFree(g.dstage[i]);
    if (g.done[i]) (void)hipEventDestroy(g.done[i]);
    g.pin[i] = nullptr; g.dstage[i] = nullptr; g.done[i] = nullptr;
  }
  if (g.st) (void)hipStreamDestroy(g.st);
  g.st = nullptr;
  g.active = false;
  idx->staging_pending.store(false);
}

void index_destroy(svs_index* idx) {
  (void)hipSetDevice(idx->device);
  staging_free(idx);
  for (AheadPipe* p : idx->pipes) pipe_destroy(p);   // (before the rows go: drains their passes and selection chains)
  for (Ctx* c : idx->free_ctx) ctx_destroy(c);
  for (auto& t : idx->evs) ev_destroy(t);
  (void)hipFree(idx->rows);
  (void)hipFree(idx->row_scales);
  for (uint32_t* col : idx->cols) (void)hipFree(col);
  (void)hipFree(idx->pfx_rows);
  (void)hipFree(idx->pfx_scales);
  (void)hipFree(idx->shadow);
  (void)hipFree(idx->scr_dev);
  if (idx->scr_host) (void)hipHostFree(idx->scr_host);
  delete idx;   // (and its owned buffers)
}

// The shadow's `bad` flag after a staging commit's conversion has drained (caller holds stg_mu, stream synchronised).
void shadow_refresh_stats(svs_index* idx) {
  if (!idx->stats_dirty) return;
  idx->stats_dirty = false;
  ScreenStats h{};
  if (idx->scr_dev && hipMemcpy(&h, idx->scr_dev, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
    if (h.bad) idx->shadow_bad.store(true);
  } else {
    (void)hipGetLastError();
    idx->shadow_bad.store(true);   // (unknown statistics: never screen on them)
  }
  idx->geo_epoch.fetch_add(1);
}

// svs_index_staging_commit publishes idx->n while its H2D copy and conversion are still queued on the staging
// stream: EVERY entry point that reads idx->rows (searches, scores, pairwise, debug read-back) waits here first.
int staging_wait(svs_index* idx) {
  if (!idx->staging_pending.load()) return SVS_OK;
  std::lock_guard<std::mutex> lk(idx->stg_mu);
  if (idx->stg.st) HIP_TRY(hipStreamSynchronize(idx->stg.st));
  shadow_refresh_stats(idx);
  idx->staging_pending.store(false);
  return SVS_OK;
}

// `want`: the stream the caller will enqueue on (nullptr = the context's own).
int ctx_acquire(svs_index* idx, hipStream_t want, bool own_stream, Ctx** out) {
  Ctx* c = nullptr;
  {
    std::unique_lock<std::mutex> lk(idx->mu);
    for (;;) {
      int pick = -1;
      for (int i = (int)idx->free_ctx.size() - 1; i >= 0; --i) {
        Ctx* f = idx->free_ctx[i];
        if (own_stream ? !f->async_pending : (f->async_pending && f->last_stream == want)) {
          pick = i;
          break;
        }
      }
      if (pick < 0 && idx->n_ctx < svs_index::kMaxCtx) {
        const int slot = idx->n_ctx++;
        lk.unlock();
        c = new (std::nothrow) Ctx();
        if (c) c->slot = slot;
        hipError_t e = c ? hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) : hipErrorOutOfMemory;
        if (e != hipSuccess) {
          ctx_destroy(c);
          lk.lock();
          idx->n_ctx--;
          return fail(SVS_ERR_DEVICE, "search context: %s", hipGetErrorString(e));
        }
        *out = c;
        return SVS_OK;
      }
      if (pick < 0 && !idx->free_ctx.empty()) pick = (int)idx->free_ctx.size() - 1;
      if (pick >= 0) {
        c = idx->free_ctx[pick];
        idx->free_ctx.erase(idx->free_ctx.begin() + pick);
        break;
      }
      idx->cv.wait(lk);
    }
  }
  // migrating between streams: drain the previous user of this scratch (rare)
  if (c->async_pending && (own_stream || c->last_stream != want)) {
    (void)hipStreamSynchronize(c->last_stream);  // a destroyed stream has already drained
    c->async_pending = false;
  }
  *out = c;
  return SVS_OK;
}

void ctx_release(svs_index* idx, Ctx* c) {
  {
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->free_ctx.push_back(c);
  }
  idx->cv.notify_one();
}

int64_t next_pow2_i64(int64_t v) {
  int64_t p = 2;
  while (p < v) p <<= 1;
  return p;
}

constexpr size_t dtype_bytes(int dtype) { return dtype == SVS_DTYPE_F32 ? 4 : (dtype == SVS_DTYPE_F16 ? 2 : 1); }
size_t elem_bytes(const svs_index* idx) { return dtype_bytes(idx->dtype); }

// ---- launch rules that several kernel families share ---------------------------------------------------
template <int N>
using Int = std::integral_constant<int, N>;

// f(std::true_type) or f(std::false_type): a run-time flag as a template argument (`flag()` is a constant in f)
template <class F>
auto with_bool(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// f(Int<n>) for n in 1 .. sizeof...(I): a run-time step count as a template argument; false: n is outside
template <class F, int... I>
bool for_steps(int n, F&& f, std::integer_sequence<int, I...>) {
  return ((n == I + 1 && (f(Int<I + 1>{}), true)) || ...);
}

// f(Int<T>): the lanes that share a row of `units` 16-byte (generic kernels: their own) units -- the smallest
// power of two that covers it, 64 (a whole wave, looping) beyond
template <class F>
void for_width(int units, F&& f) {
  if (units <= 1) f(Int<1>{});
  else if (units <= 2) f(Int<2>{});
  else if (units <= 4) f(Int<4>{});
  else if (units <= 8) f(Int<8>{});
  else if (units <= 16) f(Int<16>{});
  else if (units <= 32) f(Int<32>{});
  else f(Int<64>{});
}

// f(Int<T>, Int<NC>): the row geometry of the kernels that hold a whole row of ld16 16-byte units in registers
// (gemv_unrolled.h, gather.h) -- T lanes per row up to 1 KiB, then a wave per row at NC KiB-chunks per lane.
// false: rows longer than 16 KiB.  Rows per lane group (U) differ by family: unrolled_u / gather_u.
template <class F>
bool for_row_geometry(int ld16, F&& f) {
  if (ld16 <= 64) for_width(ld16, [&](auto t) { f(t, Int<1>{}); });
  else if (ld16 <= 128) f(Int<64>{}, Int<2>{});
  else if (ld16 <= 192) f(Int<64>{}, Int<3>{});
  else if (ld16 <= 256) f(Int<64>{}, Int<4>{});
  else if (ld16 <= 384) f(Int<64>{}, Int<6>{});
  else if (ld16 <= 512) f(Int<64>{}, Int<8>{});
  else if (ld16 <= 768) f(Int<64>{}, Int<12>{});
  else if (ld16 <= 1024) f(Int<64>{}, Int<16>{});
  else return false;
  return true;
}
constexpr int unrolled_u(int nc) { return nc <= 1 ? 8 : (nc <= 2 ? 4 : (nc <= 4 ? 2 : 1)); }
// (12-16 KiB of row loads in flight per wave: the gather rates of random whole rows need several rows per wave)
constexpr int gather_u(int nc) { return nc <= 1 ? 8 : (nc <= 2 ? 6 : (nc <= 3 ? 4 : (nc <= 4 ? 3 : (nc <= 8 ? 2 : 1)))); }

// Queries per tile of the tiled / phased kernels (f16, fp8) for a batch of nq, and so the padding of its staged image
constexpr int query_tile(int nq) { return nq <= 32 ? 32 : (nq <= 64 ? 64 : (nq <= 128 ? 128 : 256)); }

// ---- svs_index_set_variant: A/B forms of the launch rules.  Tests, tools and bench.py --variant pass the NUMBERS. ----
//  value  acts in               effect
//   0     (everywhere)          the measured defaults; the only value under which plan_search screens on its own rule
//   1     launch_rows           f32 gemv over whole wave loads: persistent grid, 1 row per wave, temporal loads
//         svs_index_top_pairs   the tiled pair path whatever n
//   2     launch_rows           persistent grid, 2 rows per wave
//         phased_ok             false: no phased kernel (the tiled kernels take its batches)
//   3     launch_rows           one-shot, 2 rows x 16 waves
//         launch_q16            f32: gemm_f32_q16_kernel (16x16x4 MFMA, half-line loads) for gemm_q16r_kernel
//   4     launch_rows           one-shot, 1 row x 16 waves, temporal loads
//         single_route          no gemv_unrolled kernels, any dtype: the generic kernels take those rows
//         launch_q16_kernel     2048 rows per workgroup (default 1024)
//         batch_route           f32: 32-query tiles whatever nq
//         launch_tiled_eb       f16 / fp8: no 128-query phased kernel; 128-row tiles (BM = TG_BM) at 128 / 256 queries per tile
//   5     launch_rows           one-shot, 1 row x 8 waves
//         launch_q16_kernel     512 rows per workgroup
//         batch_route           f16 batches never take the q16 kernel; f32 batches take it whatever nq, never the tiled kernel
//   6     plan_search           no fused epilogue
//   7     batch_route           no batched kernels, a per-query gemv loop
//   8     launch_tiled_eb       fused phased kernel: LDS-DMA pieces issued with the fragment reads (EXP 30)
//   9     launch_tiled_eb       fused phased kernel: epilogue with a branch per register (EXP 31), never the nontemporal form
//  10     launch_tiled_eb       fused phased kernel: nontemporal corpus pieces (EXP 20) with several query tiles too
//  11     plan_search           never screens
//  12     plan_search           screens whatever n
//  Any value but 0 and 12 also keeps plan_search from screening.
enum Variant : int {
  VARIANT_DEFAULT = 0,
  VARIANT_GEMV_PERSISTENT_R1 = 1,
  VARIANT_GEMV_PERSISTENT_R2 = 2,
  VARIANT_GEMV_2X16 = 3,
  VARIANT_ALT_GEOMETRY = 4,
  VARIANT_GEMV_1X8 = 5,
  VARIANT_NO_FUSION = 6,
  VARIANT_NO_BATCH_KERNELS = 7,
  VARIANT_PHASED_DMA_WITH_READS = 8,
  VARIANT_PHASED_BRANCHY_EPILOGUE = 9,
  VARIANT_PHASED_NONTEMPORAL = 10,
  VARIANT_SCREEN_OFF = 11,
  VARIANT_SCREEN_FORCE = 12,
  VARIANT_LAST = VARIANT_SCREEN_FORCE,
};

// ---- score stage launch -----------------------------------------------------
template <int NSTEP, int R, int WPB, bool NT>
void launch_oneshot(const svs_index* idx, const float* q, float* scores, hipStream_t st, const PassOpts& o) {
  const int64_t rows_per_block = (int64_t)R * WPB;
  const int64_t blocks = (idx->n + rows_per_block - 1) / rows_per_block;
  static constexpr KernelName name = kernel_name("gemv_f32_oneshot_kernel", NSTEP, R, WPB, NT, false, false);
  launch_single(o, name.s, idx->n, gemv_f32_oneshot_kernel<NSTEP, R, WPB, NT, false>, dim3((unsigned)blocks), dim3(WPB * 64), 0, st,
                (const v4f*)idx->rows, (const v4f*)q, scores, idx->n);
}

template <int NSTEP, int R, bool NT>
void launch_persistent(const svs_index* idx, const float* q, float* scores, hipStream_t st, const PassOpts& o) {
  constexpr int WPB = 4;
  const int64_t tiles = (idx->n + R - 1) / R;
  const int blocks = (int)std::min<int64_t>((tiles + WPB - 1) / WPB, (int64_t)idx->cu_count * 4);
  static constexpr KernelName name = kernel_name("gemv_f32_rows_kernel", NSTEP, R, WPB, NT, false);
  launch_single(o, name.s, idx->n, gemv_f32_rows_kernel<NSTEP, R, WPB, NT, false>, dim3(blocks), dim3(WPB * 64), 0, st,
                (const v4f*)idx->rows, (const v4f*)q, scores, idx->n);
}

// Default geometry per row length (measured at NSTEP = 6: one-shot, 16-wave
// workgroups, one row per wave, nontemporal loads: 7.2 TB/s on MI355X).
// Short rows take several rows per wave so a wave still has >= 4 KiB in flight.
// The fused f32 kernels of combine.h take the same geometry.
constexpr int f32_rows_r(int nstep) { return nstep <= 2 ? 4 : (nstep <= 4 ? 2 : 1); }
constexpr int f32_rows_wpb(int nstep) { return nstep <= 6 ? 16 : 8; }
// f(Int<NSTEP>) for the f32 one-shot kernels of rows of nstep x 256 floats; false: they have none
template <class F>
bool for_f32_rows(int nstep, F&& f) { return for_steps(nstep, f, std::make_integer_sequence<int, 16>{}); }
template <int NSTEP>
void launch_rows(const svs_index* idx, const float* q, float* scores, hipStream_t st, int variant, const PassOpts& o) {
  switch (variant) {
    case VARIANT_GEMV_PERSISTENT_R1: launch_persistent<NSTEP, 1, false>(idx, q, scores, st, o); return;
    case VARIANT_GEMV_PERSISTENT_R2: launch_persistent<NSTEP, 2, true>(idx, q, scores, st, o); return;
    case VARIANT_GEMV_2X16: launch_oneshot<NSTEP, 2, 16, true>(idx, q, scores, st, o); return;
    case VARIANT_ALT_GEOMETRY: launch_oneshot<NSTEP, 1, 16, false>(idx, q, scores, st, o); return;
    case VARIANT_GEMV_1X8: launch_oneshot<NSTEP, 1, 8, true>(idx, q, scores, st, o); return;
    default: break;
  }
  launch_oneshot<NSTEP, f32_rows_r(NSTEP), f32_rows_wpb(NSTEP), true>(idx, q, scores, st, o);
}

// The grid of the loop kernels: T lanes per row, four waves per workgroup, at most eight workgroups per CU
template <int T>
int loop_blocks(const svs_index* idx) {
  return (int)std::min<int64_t>(((idx->n + 64 / T - 1) / (64 / T) + 3) / 4, (int64_t)idx->cu_count * 8);
}

template <int T>
void launch_generic(const svs_index* idx, const float* q, float* scores, hipStream_t st, const PassOpts& o) {
  static constexpr KernelName name = kernel_name("gemv_f32_generic_kernel", T);
  launch_single(o, name.s, idx->n, gemv_f32_generic_kernel<T>, dim3(loop_blocks<T>(idx)), dim3(256), 0, st,
                (const v4f*)idx->rows, q, scores, idx->n, idx->d, idx->ld / 4);
}

constexpr int f16_rows_r(int nstep) { return nstep <= 1 ? 4 : (nstep <= 3 ? 2 : 1); }
constexpr int f16_rows_wpb(int nstep) { return nstep <= 6 ? 16 : 8; }
template <int NSTEP>
constexpr KernelName kF16OneshotName = kernel_name("gemv_f16_oneshot_kernel", NSTEP, f16_rows_r(NSTEP), f16_rows_wpb(NSTEP));
// dynamic LDS of a launch under a plan: the plan's queries as halves (gemv_f16.h), at most 4 x 3584 x 2 = 28 KB
inline unsigned plan_lds_bytes(int limit, int ld) { return (unsigned)limit * (unsigned)ld * 2u; }
// The thin grid of an instantiation: as many workgroups as the device holds at once (with the LDS of a full plan).
template <int NSTEP>
int thin_grid_rows_f16(const svs_index* idx) {
  constexpr int R = f16_rows_r(NSTEP), WPB = f16_rows_wpb(NSTEP);
  static std::atomic<int> per_cu{0};
  int v = per_cu.load(std::memory_order_relaxed);
  if (!v) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gemv_f16_oneshot_kernel<NSTEP, R, WPB>, WPB * 64,
                                                     (size_t)plan_lds_bytes(SHARE_MAX, NSTEP * 512)) != hipSuccess || nb < 1) {
      (void)hipGetLastError();
      nb = 1;
    }
    per_cu.store(v = nb, std::memory_order_relaxed);
  }
  return idx->cu_count * v;
}
// f(Int<NSTEP>) for the f16 one-shot kernel of rows of nstep x 512 halves; false: it has none
template <class F>
bool for_f16_oneshot(int nstep, F&& f) { return for_steps(nstep, f, std::make_integer_sequence<int, 8>{}); }
// ... of the index's shareable passes (0: its row length does not share)
int thin_grid_of(const svs_index* idx) {
  int grid = 0;
  if (idx->ld % 512 == 0) for_f16_oneshot(idx->ld / 512, [&](auto ns) { if constexpr (f16_rows_share(ns())) grid = thin_grid_rows_f16<ns()>(idx); });
  return grid;
}
// half_rows: half_rows_of the route; o.plan: the plan the launch serves (a geometry that shares), else its own q and scores
template <int NSTEP>
void launch_rows_f16(const svs_index* idx, const void* half_rows, const float* q, float* scores, hipStream_t st, const PassOpts& o) {
  constexpr int R = f16_rows_r(NSTEP), WPB = f16_rows_wpb(NSTEP);
  const int64_t rows_per_block = (int64_t)R * WPB;
  int64_t blocks = (idx->n + rows_per_block - 1) / rows_per_block;
  const PassPlan* plan = f16_rows_share(NSTEP) ? o.plan : nullptr;
  if constexpr (f16_rows_share(NSTEP))
    if (plan && o.thin) blocks = std::min<int64_t>(blocks, thin_grid_rows_f16<NSTEP>(idx));
  launch_single(o, kF16OneshotName<NSTEP>.s, idx->n, gemv_f16_oneshot_kernel<NSTEP, R, WPB>, dim3((unsigned)blocks), dim3(WPB * 64),
                plan ? plan_lds_bytes(o.limit, NSTEP * 512) : 0u, st, (const u32x4*)half_rows, (const v4f*)q, scores, idx->n, plan);
}

template <int T>
void launch_generic_f16(const svs_index* idx, const _Float16* qh, float* scores, hipStream_t st, const PassOpts& o) {
  static constexpr KernelName name = kernel_name("gemv_f16_generic_kernel", T);
  launch_single(o, name.s, idx->n, gemv_f16_generic_kernel<T>, dim3(loop_blocks<T>(idx)), dim3(256), 0, st, (const u32x4*)idx->rows,
                (const u32x4*)qh, scores, idx->n, idx->ld / 8);
}

// rounds nq f32 queries to half into c->qh ([rows_alloc][ld], rows >= nq zero)
// (row0 > 0: a later chunk of a batch staged piece by piece -- search_host; the buffer was grown by the first chunk's
//  call, which passes the whole batch's row count as rows_alloc, and only the last chunk zeroes the padding rows)
int stage_queries_f16(const svs_index* idx, Ctx* c, const float* q, int nq, int rows_alloc, hipStream_t st, int row0 = 0) {
  int rc = c->qh.grow((size_t)rows_alloc * idx->ld);
  if (rc != SVS_OK) return rc;
  _Float16* dst = c->qh + (size_t)row0 * idx->ld;
  rows_alloc -= row0;
  // (the kernel writes whole padded rows: only the rows behind the queries need zeroing)
  if (rows_alloc > nq) HIP_TRY(hipMemsetAsync(dst + (size_t)nq * idx->ld, 0, (size_t)(rows_alloc - nq) * idx->ld * sizeof(_Float16), st));
  hipLaunchKernelGGL(convert_queries_f16_kernel, dim3((unsigned)std::min<int64_t>(2048, ((int64_t)nq * idx->ld + 255) / 256)), dim3(256), 0, st, q, nq, idx->d, dst, idx->ld);
  return SVS_OK;
}

// quantises nq f32 queries to e4m3 into c->q8 ([rows_alloc][ld] bytes, rows >= nq zero) with
// scales c->q8s; want_f32 also fills c->q8f with the quantised values as f32
int stage_queries_fp8(const svs_index* idx, Ctx* c, const float* q, int nq, int rows_alloc, bool want_f32, hipStream_t st) {
  int rc;
  if ((rc = c->q8.grow((size_t)rows_alloc * idx->ld)) != SVS_OK) return rc;
  if ((rc = c->q8s.grow((size_t)rows_alloc)) != SVS_OK) return rc;
  if (want_f32 && (rc = c->q8f.grow((size_t)rows_alloc * idx->ld)) != SVS_OK) return rc;
  if (rows_alloc > nq) {   // (the kernel writes whole padded rows: only the rows behind the queries need zeroing)
    HIP_TRY(hipMemsetAsync(c->q8 + (size_t)nq * idx->ld, 0, (size_t)(rows_alloc - nq) * idx->ld, st));
    HIP_TRY(hipMemsetAsync(c->q8s + nq, 0, (size_t)(rows_alloc - nq) * sizeof(float), st));
  }
  hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3((nq + 3) / 4), dim3(256), 0, st, q, (int64_t)nq, idx->d, (int64_t)idx->d,
                     c->q8, idx->ld, c->q8s, want_f32 ? c->q8f : (float*)nullptr);
  return SVS_OK;
}

template <int T>
void launch_gemv_fp8(const svs_index* idx, const Ctx* c, float* scores, hipStream_t st, const PassOpts& o) {
  static constexpr KernelName name = kernel_name("gemv_fp8_kernel", T);
  launch_single(o, name.s, idx->n, gemv_fp8_kernel<T>, dim3(loop_blocks<T>(idx)), dim3(256), 0, st, (const u32x4_t*)idx->rows, idx->row_scales,
                (const v4f*)c->q8f.p, c->q8s.p, scores, idx->n, idx->ld / 16);
}

// f(Int<NSTEP>, Int<LB>, Int<R>) for the hot row lengths (bytes): one-shot grid, 16 waves, nontemporal row loads.  The
// query stays packed, so several short rows per wave cost no registers (58-66 VGPRs).  false: not one of them
template <class F>
bool for_fp8_oneshot(int ld, F&& f) {
  switch (ld) {
    case 1024: f(Int<1>{}, Int<16>{}, Int<4>{}); return true;   // >= 4 KiB per wave: 6.5 vs 4.2 TB/s with one row per wave
    case 2048: f(Int<2>{}, Int<16>{}, Int<2>{}); return true;   // 6.5 vs 5.8
    case 3072: f(Int<3>{}, Int<16>{}, Int<1>{}); return true;
    case 4096: f(Int<4>{}, Int<16>{}, Int<1>{}); return true;
    case 512: f(Int<1>{}, Int<8>{}, Int<4>{}); return true;     // 8-byte loads: several rows per wave keep enough bytes in flight
    case 1536: f(Int<3>{}, Int<8>{}, Int<2>{}); return true;
    default: return false;
  }
}
template <int NSTEP, int LB, int R>
void launch_oneshot_fp8(const svs_index* idx, const Ctx* c, float* scores, hipStream_t st, const PassOpts& o) {
  static constexpr KernelName name = kernel_name("gemv_fp8_oneshot_kernel", NSTEP, LB, R, 16);
  launch_single(o, name.s, idx->n, gemv_fp8_oneshot_kernel<NSTEP, LB, R, 16>, dim3((unsigned)((idx->n + R * 16 - 1) / (R * 16))), dim3(16 * 64), 0, st,
                (const uint8_t*)idx->rows, idx->row_scales, (const uint8_t*)c->q8.p, c->q8s.p, scores, idx->n);
}

// The Dot argument of gemv_unrolled_kernel as c++filt prints it
template <class Dot> constexpr const char* kDotName = nullptr;
template <> constexpr const char* kDotName<DotF32> = "svs::DotF32";
template <> constexpr const char* kDotName<DotF16> = "svs::DotF16";
template <> constexpr const char* kDotName<DotFp8> = "svs::DotFp8";

// Rows that are not whole 1 KiB wave loads (gemv_unrolled.h); false: longer than 16 KiB
template <class Dot>
bool launch_unrolled(const svs_index* idx, const void* q_staged, int ld16, float* scores, hipStream_t st, Dot dot, const PassOpts& o) {
  const u32x4* M = (const u32x4*)idx->rows;
  const u32x4* q = (const u32x4*)q_staged;
  return for_row_geometry(ld16, [&](auto t, auto nc) {
    constexpr int T = t(), NC = nc(), U = unrolled_u(NC);
    const int64_t groups = (idx->n + (64 / T) * U - 1) / ((64 / T) * U);
    const int64_t blocks = (groups + UNR_WPB - 1) / UNR_WPB;
    static constexpr KernelName name = kernel_name("gemv_unrolled_kernel", T, NC, U, kDotName<Dot>);
    launch_single(o, name.s, idx->n, gemv_unrolled_kernel<T, NC, U, Dot>, dim3((unsigned)blocks), dim3(UNR_WPB * 64), 0, st, M, q, scores, idx->n, ld16, dot);
  });
}

// ---- the route of a single query: decided once (single_route), then staged and launched from that value ----------
struct SingleRoute {
  enum Family : uint8_t { F32_ROWS, F32_UNROLLED, F32_GENERIC, F16_ONESHOT, F16_UNROLLED, F16_GENERIC, FP8_ONESHOT, FP8_UNROLLED, FP8_GENERIC } family;
  // the query as the kernel reads it: the caller's d floats; ld floats, 16-byte aligned (the caller's, or pad_query's
  // zero-padded copy in Ctx::q16); halves in Ctx::qh; e4m3 in Ctx::q8 with its scale in q8s and the values as f32 in q8f
  enum Query : uint8_t { AS_GIVEN, PADDED, HALF, FP8 } query;
  bool shadow;   // the rows it reads: idx->shadow (a screened f32 index takes F16_ONESHOT over it), else idx->rows
  bool shares;   // its pass can serve other searches of a run-ahead pipeline (pass_share.h)
  int geo;       // template geometry: NSTEP of the one-shot / persistent kernels, else 16-byte chunks per row
  int variant;   // svs_index_set_variant when the route was taken (F32_ROWS, launch_rows: one-shot or persistent grid, R x WPB, loads)
};

// variant: idx->variant, loaded ONCE by whoever plans the search; screen: the search runs over the half shadow
SingleRoute single_route(const svs_index* idx, int variant, bool screen) {
  using R = SingleRoute;
  const int ld = idx->ld;
  const auto none = [](auto...) {};
  // other rows of up to 16 KiB: gemv_unrolled.h (f32: the query in 16-byte chunks of the padded row); else the loop kernels
  const auto unrolled = [&](int ld16) { return variant != VARIANT_ALT_GEOMETRY && for_row_geometry(ld16, none); };
  if (idx->dtype == SVS_DTYPE_FP8)
    return R{for_fp8_oneshot(ld, none) ? R::FP8_ONESHOT : (unrolled(ld / 16) ? R::FP8_UNROLLED : R::FP8_GENERIC), R::FP8, false, false, ld / 16, variant};
  if (screen || (idx->dtype == SVS_DTYPE_F16 && ld % 512 == 0 && ld <= 4096))   // (the kernel rounds ld query floats itself)
    return R{R::F16_ONESHOT, R::PADDED, screen, f16_rows_share(ld / 512), ld / 512, variant};
  if (idx->dtype == SVS_DTYPE_F16) return R{unrolled(ld / 8) ? R::F16_UNROLLED : R::F16_GENERIC, R::HALF, false, false, ld / 8, variant};
  if (ld % 256 == 0 && ld <= 4096) return R{R::F32_ROWS, R::PADDED, false, false, ld / 256, variant};   // (the kernel reads ld query floats)
  return unrolled(ld / 4) ? R{R::F32_UNROLLED, R::PADDED, false, false, ld / 4, variant} : R{R::F32_GENERIC, R::AS_GIVEN, false, false, ld / 4, variant};
}

// The rows a route's pass reads: the half shadow (screened f32 index) or the index's own
inline const void* half_rows_of(const svs_index* idx, const SingleRoute& r) { return r.shadow ? idx->shadow : idx->rows; }

// The route's kernel over q, the query staged as r.query says (FP8: in the context).  o.name: the kernel is named, not launched.
int launch_route(const svs_index* idx, const Ctx* c, const SingleRoute& r, const void* q, float* scores, hipStream_t st, const PassOpts& o) {
  bool ok = true;
  switch (r.family) {
    case SingleRoute::FP8_ONESHOT: ok = for_fp8_oneshot(idx->ld, [&](auto ns, auto lb, auto rr) { launch_oneshot_fp8<ns(), lb(), rr()>(idx, c, scores, st, o); }); break;
    case SingleRoute::FP8_UNROLLED: ok = launch_unrolled(idx, q, r.geo, scores, st, DotFp8{idx->row_scales, c->q8s}, o); break;
    case SingleRoute::FP8_GENERIC: for_width(r.geo, [&](auto t) { launch_gemv_fp8<t()>(idx, c, scores, st, o); }); break;
    case SingleRoute::F16_ONESHOT: ok = for_f16_oneshot(r.geo, [&](auto ns) { launch_rows_f16<ns()>(idx, half_rows_of(idx, r), (const float*)q, scores, st, o); }); break;
    case SingleRoute::F16_UNROLLED: ok = launch_unrolled(idx, q, r.geo, scores, st, DotF16{}, o); break;
    case SingleRoute::F16_GENERIC: for_width(r.geo, [&](auto t) { launch_generic_f16<t()>(idx, (const _Float16*)q, scores, st, o); }); break;
    case SingleRoute::F32_ROWS: ok = for_f32_rows(r.geo, [&](auto ns) { launch_rows<ns()>(idx, (const float*)q, scores, st, r.variant, o); }); break;
    case SingleRoute::F32_UNROLLED: ok = launch_unrolled(idx, q, r.geo, scores, st, DotF32{}, o); break;
    case SingleRoute::F32_GENERIC: for_width(r.geo, [&](auto t) { launch_generic<t()>(idx, (const float*)q, scores, st, o); }); break;
  }
  return ok ? SVS_OK : fail(SVS_ERR_INVALID, "internal: no single-query kernel for ld %d", idx->ld);
}

// The query as the single-query kernels read it: ld floats, 16-byte aligned.  Copied (zero padded) when the rows are
// padded beyond d or the pointer is not aligned
inline bool query_needs_copy(const svs_index* idx, const float* q) { return idx->ld != idx->d || (((uintptr_t)q) & 15) != 0; }
int pad_query(const svs_index* idx, Ctx* c, const float* q, const float** out, hipStream_t st) {
  *out = q;
  if (!query_needs_copy(idx, q)) return SVS_OK;
  int rc = c->q16.grow((size_t)GQ * idx->ld);
  if (rc != SVS_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->q16, 0, (size_t)idx->ld * sizeof(float), st));
  HIP_TRY(hipMemcpyAsync(c->q16, q, (size_t)idx->d * sizeof(float), hipMemcpyDeviceToDevice, st));
  *out = c->q16;
  return SVS_OK;
}

// One query through its route.  q: device, d floats; scores: n floats; q_padded (may be null): the query a PADDED route read
int launch_scores(const svs_index* idx, Ctx* c, const SingleRoute& r, const float* q, float* scores, hipStream_t st,
                  const PassOpts& o = {}, const float** q_padded = nullptr) {
  const float* qq = q;
  const int rc = r.query == SingleRoute::PADDED ? pad_query(idx, c, q, &qq, st)
                 : r.query == SingleRoute::HALF ? stage_queries_f16(idx, c, q, 1, 1, st)
                 : r.query == SingleRoute::FP8  ? stage_queries_fp8(idx, c, q, 1, 1, true, st) : SVS_OK;
  if (rc != SVS_OK) return rc;
  if (q_padded) *q_padded = qq;
  const void* staged = r.query == SingleRoute::HALF ? (const void*)c->qh.p : (r.query == SingleRoute::FP8 ? (const void*)c->q8.p : (const void*)qq);
  return launch_route(idx, c, r, staged, scores, st, o);
}

// ---- the route of a batch (two or more queries): decided once per call (batch_route), staged once (stage_batch),
// ---- launched pass by pass (launch_batch) ------------------------------------------------------------------------
struct BatchRoute {
  // the per-query loop of the single-query kernels (`single`), the 16-query kernels (gemm_q16.h), the f32 tiled kernel,
  // the f16 / fp8 tiled and phased kernels (gemm_tiled.h, gemm_phased.h)
  enum Family : uint8_t { LOOP, Q16, TILED_F32, TILED_EB } family = LOOP;
  // the queries as the family's kernels read them, [rows()][ld] zero padded: f32 (the caller's buffer where it has that
  // shape, else Ctx::q16), halves in Ctx::qh, e4m3 in Ctx::q8 with their scales in q8s; LOOP: launch_scores stages each
  enum Query : uint8_t { PER_QUERY, PADDED_F32, HALF, FP8 } query = PER_QUERY;
  int nq = 0;
  int tile = 1;           // queries per group (Q16: GQ) or query tile (f32: 32 / 64; f16, fp8: query_tile(nq)); LOOP: 1
  int variant = 0;        // svs_index_set_variant when the route was taken: every pass's launcher decides by THIS value
  SingleRoute single{};   // LOOP: the route of each query
  int rows() const { return (nq + tile - 1) / tile * tile; }   // rows of the staged image: the one statement of its padding
};

// variant: idx->variant, loaded ONCE by the entry point.  What depends on the pass -- fused or not, pair mode, phased or
// tiled (phased_ok: n_rows) -- is resolved by launch_batch from the route and the pass's own arguments.
BatchRoute batch_route(const svs_index* idx, int variant, int nq) {
  using R = BatchRoute;
  const int ld = idx->ld;
  const bool f32 = idx->dtype == SVS_DTYPE_F32, f16 = idx->dtype == SVS_DTYPE_F16;
  const bool kernels = nq >= 2 && variant != VARIANT_NO_BATCH_KERNELS;
  // 16-query kernels: the query image (16 x row bytes) must fit the LDS beside the fused candidate list (f16: rows of
  // whole pairs of 256-byte steps); tiled kernels: rows of whole 128-byte k-tiles (f32: not under variant 5, A/B)
  const bool q16 = kernels && (f32 ? ld % 128 == 0 && ld <= 2304 : f16 && ld % 256 == 0 && ld <= 4608);
  const bool tiled = kernels && ((size_t)ld * elem_bytes(idx)) % TG_BKB == 0 && !(f32 && variant == VARIANT_GEMV_1X8);
  const R::Query staged = f32 ? R::PADDED_F32 : (f16 ? R::HALF : R::FP8);
  // up to 16 queries; f32 also every batch the tiled kernel does not take; f16 under variant 5 never (tiled kernel, A/B)
  if (q16 && (f32 ? nq <= GQ || !tiled : nq <= GQ && variant != VARIANT_GEMV_1X8)) return R{R::Q16, staged, nq, GQ, variant};
  if (!tiled) return R{R::LOOP, R::PER_QUERY, nq, 1, variant, single_route(idx, variant, false)};
  // exact-f32 MFMA runs at the vector rate: 32 queries per pass keep the kernel HBM-bound (62 % of the matrix pipe);
  // larger batches are more query tiles of the same launch (grid y).  64 queries per tile from 33 queries up (256
  // queries: 6.7 vs 7.3 ms with 32; 128-query tiles measured the same as 64: ~125 TFLOP/s of the 157 TF f32 MFMA peak)
  if (f32) return R{R::TILED_F32, staged, nq, nq > 32 && variant != VARIANT_ALT_GEOMETRY ? 64 : 32, variant};   // (32-query tiles, A/B)
  return R{R::TILED_EB, staged, nq, query_tile(nq), variant};
}

struct FuseLaunch {   // non-null state: fused top-k epilogue, no score matrix
  uint32_t* state = nullptr;
  uint64_t* cand = nullptr;
  const float* thr = nullptr;   // thr[q * thr_stride]: lower bound of query q's k-th best score
  int thr_stride = 0;
  TgPairs pairs{};              // pair mode (svs_index_top_pairs, tiled kernels only): see gemm_tiled.h
  const void* rows = nullptr;   // non-null: the row operand is THIS matrix (the prefix image), not idx->rows
  const float* row_scales = nullptr;   // ... and its fp8 row scales
  FuseLaunch at(int q0) const {
    if (!state) return *this;
    return FuseLaunch{state + (size_t)q0 * SCR_WORDS, cand + (size_t)q0 * CAND_CAP, thr + (size_t)q0 * thr_stride, thr_stride, pairs, rows, row_scales};
  }
  const void* rows_of(const svs_index* idx) const;
  const float* scales_of(const svs_index* idx) const;
};

inline const void* FuseLaunch::rows_of(const svs_index* idx) const { return rows ? rows : idx->rows; }
inline const float* FuseLaunch::scales_of(const svs_index* idx) const { return rows ? row_scales : idx->row_scales; }

// f32 queries as the batched kernels read them: [nq_pad][ld], zero padded (rows >= nq zero).
// Returns the caller's buffer itself when it already has that shape.
int stage_queries_f32(const svs_index* idx, Ctx* c, const float* q_dev, int nq, int nq_pad, const float** out, hipStream_t st) {
  const int ld = idx->ld;
  if (nq_pad == nq && ld == idx->d && !(((uintptr_t)q_dev) & 15)) { *out = q_dev; return SVS_OK; }
  int rc = c->q16.grow((size_t)nq_pad * ld);
  if (rc != SVS_OK) return rc;
  HIP_TRY(hipMemsetAsync(c->q16, 0, (size_t)nq_pad * ld * sizeof(float), st));
  HIP_TRY(hipMemcpy2DAsync(c->q16, (size_t)ld * sizeof(float), q_dev, (size_t)idx->d * sizeof(float),
                           (size_t)idx->d * sizeof(float), (size_t)nq, hipMemcpyDeviceToDevice, st));
  *out = c->q16;
  return SVS_OK;
}

template <bool FUSE, int EB>
constexpr KernelName kQ16rName = kernel_name("gemm_q16r_kernel", FUSE, EB, G4_RG, G4_PF);
template <bool FUSE>
constexpr KernelName kF32Q16Name = kernel_name("gemm_f32_q16_kernel", false, 2, GEMM_PF, FUSE);

// What a batched pass is launched with besides the route: the staged queries, the row range, where the scores go
// (null with fl.state: the fused epilogue keeps candidates instead), and name -- the kernel is named, not launched
struct BatchPass {
  const void* q;
  int64_t n_rows;
  float* scores;
  int64_t sstride;
  FuseLaunch fl;
  hipStream_t st;
  const char** name;
};

// ---- up to 16 queries per corpus pass (gemm_q16.h) ---------------------------
// One group: q16 = 16 staged queries ([16][ld] in the corpus dtype: f32, or halves for an f16 corpus), nq_g of them real
template <auto Kernel, class P>
void launch_q16_kernel(const char* name, const svs_index* idx, int variant, const void* q16, int ld_units, int nq_g, float* scores,
                       const FuseLaunch& fl, const BatchPass& p) {
  // 1024 rows (6 MB at d = 1536) per workgroup amortise the 96 KiB query staging; short
  // row ranges (the fused path's prefix) take smaller blocks so that every CU gets one.
  int rows_per_block = variant == VARIANT_ALT_GEOMETRY ? 2048 : (variant == VARIANT_GEMV_1X8 ? 512 : 1024);
  while (rows_per_block > 64 && (p.n_rows + rows_per_block - 1) / rows_per_block < 512) rows_per_block /= 2;
  const unsigned blocks = (unsigned)((p.n_rows + rows_per_block - 1) / rows_per_block);
  const size_t row_bytes = (size_t)idx->ld * elem_bytes(idx);
  const size_t lds = row_bytes * 16 + (fl.state ? GEMM_FUSE_LDS : 0);   // 16 queries x row bytes
  launch_batched<Kernel>(p.name, name, 2304 * 64 + GEMM_FUSE_LDS, p.n_rows, nq_g, dim3(blocks), dim3(GEMM_WAVES * 64), lds, p.st,
                         (const P*)fl.rows_of(idx), (const P*)q16, scores, p.n_rows, ld_units, p.sstride, nq_g, rows_per_block,
                         fl.state, (int)SCR_WORDS, fl.cand, (uint32_t)CAND_CAP, fl.thr, fl.thr_stride);
}

// (Kernels are emitted in the order they are first named.  The six 16-query kernels are named here in the order the
//  library has always had them, so that the device code keeps its layout whatever order launch_q16 reaches them in.)
template <auto... K> struct KernelOrder {};
using Q16KernelOrder = KernelOrder<gemm_q16r_kernel<false, 4>, gemm_q16r_kernel<true, 4>, gemm_q16r_kernel<false, 2>, gemm_q16r_kernel<true, 2>,
                                   gemm_f32_q16_kernel<false, 2, GEMM_PF, false>, gemm_f32_q16_kernel<false, 2, GEMM_PF, true>>;

// The groups of 16 of a Q16 route, one launch each
void launch_q16(const svs_index* idx, const BatchRoute& r, const BatchPass& p) {
  const size_t group_bytes = (size_t)GQ * idx->ld * elem_bytes(idx);
  const int ld16 = (int)(group_bytes / GQ / 16);
  with_bool(p.fl.state != nullptr, [&](auto fuse) {
    constexpr bool F = fuse();
    for (int q0 = 0; q0 < r.nq; q0 += GQ) {
      const void* qg = (const uint8_t*)p.q + (size_t)(q0 / GQ) * group_bytes;
      float* sg = p.scores ? p.scores + (size_t)q0 * p.sstride : nullptr;
      const int nq_g = std::min(GQ, r.nq - q0);
      if (idx->dtype == SVS_DTYPE_F16)
        launch_q16_kernel<gemm_q16r_kernel<F, 2>, v4f>(kQ16rName<F, 2>.s, idx, r.variant, qg, ld16, nq_g, sg, p.fl.at(q0), p);
      else if (r.variant == VARIANT_GEMV_2X16)   // A/B: the 16x16x4 kernel (half-line loads)
        launch_q16_kernel<gemm_f32_q16_kernel<false, 2, GEMM_PF, F>, float>(kF32Q16Name<F>.s, idx, r.variant, qg, idx->ld, nq_g, sg, p.fl.at(q0), p);
      else
        launch_q16_kernel<gemm_q16r_kernel<F, 4>, v4f>(kQ16rName<F, 4>.s, idx, r.variant, qg, ld16, nq_g, sg, p.fl.at(q0), p);
      if (p.name) break;   // (named once: every group takes the same kernel)
    }
  });
}

// ---- LDS-tiled MFMA GEMM (gemm_tiled.h): f32 (EB 4), f16 (2), fp8 (1); nq queries at BN per tile ----------------------
template <int BN, bool FUSE, int EB, int BM = TG_BM>
void launch_tiled_bn(const svs_index* idx, const Ctx* c, int nq, const BatchPass& p) {
  static constexpr KernelName name = kernel_name("gemm_tiled_kernel", BN, FUSE, EB, BM);
  const FuseLaunch& fl = p.fl;
  const unsigned gx = (unsigned)((p.n_rows + BM - 1) / BM), gy = (unsigned)((nq + BN - 1) / BN);
  // pair mode: the row operand starts at global row fl.pairs.row_base (n_rows counts from there)
  const int64_t rb = fl.pairs.on ? fl.pairs.row_base : 0;
  launch_batched<gemm_tiled_kernel<BN, FUSE, EB, BM>>(
      p.name, name.s, tg_lds_bytes(BM, BN), p.n_rows, nq, dim3(gx, gy), dim3(TG_WAVES * 64), (size_t)tg_lds_bytes(BM, BN), p.st,
      (const uint8_t*)fl.rows_of(idx) + (size_t)rb * idx->ld * EB, (const uint8_t*)p.q, p.scores, p.n_rows, (int64_t)idx->ld * EB, p.sstride, nq,
      fl.state, (int)SCR_WORDS, fl.cand, (uint32_t)CAND_CAP, fl.thr, fl.thr_stride,
      (const float*)(fl.scales_of(idx) ? fl.scales_of(idx) + rb : nullptr), (const float*)c->q8s.p, fl.pairs);
}

// 256 x 256 output tiles, persistent workgroups, four-phase k-tiles (gemm_phased.h)
template <bool FUSE, int EB, int EXP = 0, int QT = PG_TILE>
void launch_phased(const svs_index* idx, const Ctx* c, int nq, const BatchPass& p) {
  static constexpr KernelName name = kernel_name("gemm_phased_kernel", FUSE, EB, EXP, QT);
  const FuseLaunch& fl = p.fl;
  const int gx = (int)((p.n_rows + PG_TILE - 1) / PG_TILE), gy = (nq + QT - 1) / QT;
  const int64_t total = (int64_t)gx * gy;
  const unsigned grid = (unsigned)std::min<int64_t>(total, idx->cu_count);   // one persistent workgroup per CU
  // pair mode: the row operand starts at global row fl.pairs.row_base (n_rows counts from there)
  const int64_t rb = fl.pairs.on ? fl.pairs.row_base : 0;
  launch_batched<gemm_phased_kernel<FUSE, EB, EXP, QT>>(
      p.name, name.s, PG_LDS_TOTAL, p.n_rows, nq, dim3(grid), dim3(PG_THREADS), (size_t)PG_LDS_TOTAL, p.st,
      (const uint8_t*)fl.rows_of(idx) + (size_t)rb * idx->ld * EB, (const uint8_t*)p.q, p.scores, p.n_rows, (int)(idx->ld * EB), p.sstride, nq, gx, gy,
      fl.state, (int)SCR_WORDS, fl.cand, (uint32_t)CAND_CAP, fl.thr, fl.thr_stride,
      (const float*)(fl.scales_of(idx) ? fl.scales_of(idx) + rb : nullptr), (const float*)c->q8s.p, fl.pairs);
}

// the phased kernel's preconditions (f16 / fp8 rows): an even number (>= 6) of 128-byte k-tiles per row, tile bytes
// and tile counts inside 32-bit descriptors / ints
bool phased_ok(const svs_index* idx, int variant, int64_t n_rows, int nq) {
  const int64_t ldb = (int64_t)idx->ld * (int64_t)elem_bytes(idx);
  return variant != VARIANT_GEMV_PERSISTENT_R2 && ldb % (2 * TG_BKB) == 0 && ldb >= PG_MIN_KT * TG_BKB && ldb <= (1 << 20) &&
         ((n_rows + PG_TILE - 1) / PG_TILE) * ((nq + PG_TILE - 1) / PG_TILE) < (1ll << 30);
}

// A TILED_EB route's pass: phased or tiled by the pass's rows, the fused forms by the route's variant
template <int EB>
void launch_tiled_eb(const svs_index* idx, const Ctx* c, const BatchRoute& r, const BatchPass& p) {
  const int variant = r.variant, nq = r.nq, bn = r.tile;
  with_bool(p.fl.state != nullptr, [&](auto fuse) {
    constexpr bool F = fuse();
    if (bn == 256 && phased_ok(idx, variant, p.n_rows, nq)) {
      if constexpr (F) {
        if (variant == VARIANT_PHASED_DMA_WITH_READS)   // A/B: LDS-DMA pieces issued with the fragment reads
          return launch_phased<true, EB, 30>(idx, c, nq, p);
        if (variant == VARIANT_PHASED_BRANCHY_EPILOGUE)   // A/B: fused epilogue with a branch per register
          return launch_phased<true, EB, 31>(idx, c, nq, p);
        // One query tile (up to 256 queries): every corpus byte is used by exactly one workgroup, so its LDS-DMA
        // pieces are issued nontemporal (EXP 20) and leave the L2 to the queries (configs[4]: 7.63 vs 7.89-8.0 ms in
        // tools/gemm_phased_bench; with several query tiles the corpus tile is SHARED through the L2: not there).
        if (nq <= PG_TILE || variant == VARIANT_PHASED_NONTEMPORAL)   // (nontemporal with several query tiles too, A/B)
          return launch_phased<true, EB, 20>(idx, c, nq, p);
      }
      return launch_phased<F, EB>(idx, c, nq, p);
    }
    // 65 .. 128 queries (one query tile: the batches a coalescer forms on a reduced-precision index): the phased
    // kernel at 128-query tiles, corpus pieces nontemporal -- HBM-bound, every corpus byte used once
    if (bn == 128 && !p.fl.pairs.on && variant != VARIANT_ALT_GEOMETRY && phased_ok(idx, variant, p.n_rows, nq))
      return launch_phased<F, EB, F ? 20 : 0, 128>(idx, c, nq, p);
    switch (bn) {
      case 32: return launch_tiled_bn<32, F, EB>(idx, c, nq, p);
      case 64:   // (256-row tiles measured 2-5 % slower here)
        return launch_tiled_bn<64, F, EB>(idx, c, nq, p);
      case 128:
        if (variant == VARIANT_ALT_GEOMETRY)   // A/B: 128-row tiles (0.87 vs 0.76 ms at 1M x 1536 f16)
          return launch_tiled_bn<128, F, EB>(idx, c, nq, p);
        return launch_tiled_bn<128, F, EB, 256>(idx, c, nq, p);
      default:
        if (variant == VARIANT_ALT_GEOMETRY)   // A/B: 128-row tiles, three-stage ring
          return launch_tiled_bn<256, F, EB>(idx, c, nq, p);
        return launch_tiled_bn<256, F, EB, 256>(idx, c, nq, p);
    }
  });
}

// The call's queries (q_dev: [nq][d] f32, device -- or device-visible for the half image) as the route's kernels read
// them, once per call.  *staged: what every pass of the call is launched with.
int stage_batch(const svs_index* idx, Ctx* c, const BatchRoute& r, const float* q_dev, hipStream_t st, const void** staged) {
  int rc = SVS_OK;
  const float* qs = q_dev;   // (PER_QUERY: launch_scores stages each query as r.single says)
  switch (r.query) {
    case BatchRoute::PER_QUERY: break;
    case BatchRoute::PADDED_F32: rc = stage_queries_f32(idx, c, q_dev, r.nq, r.rows(), &qs, st); break;
    case BatchRoute::HALF: rc = stage_queries_f16(idx, c, q_dev, r.nq, r.rows(), st); break;
    case BatchRoute::FP8: rc = stage_queries_fp8(idx, c, q_dev, r.nq, r.rows(), false, st); break;
  }
  *staged = r.query == BatchRoute::HALF ? (const void*)c->qh.p : (r.query == BatchRoute::FP8 ? (const void*)c->q8.p : (const void*)qs);
  return rc;
}

// One pass of the route over rows [0, n_rows) of the corpus (or of fl.rows).  q: the queries as stage_batch left them;
// fl.state != null: fused epilogue (batched kernels only); name (svs_internal_batch_route): the pass's kernel is named, not launched
int launch_batch(const svs_index* idx, Ctx* c, const BatchRoute& r, const void* q, int64_t n_rows, float* scores, int64_t sstride,
                 FuseLaunch fl, hipStream_t st, const char** name = nullptr) {
  const BatchPass p{q, n_rows, scores, sstride, fl, st, name};
  switch (r.family) {
    case BatchRoute::Q16:
      // The 16-query kernels have no pair mode: launch_q16_kernel does not pass fl.pairs on, so they would offer (i, i) and
      // j < i as candidates.  svs_index_top_pairs keeps corpora that form such chunks on the materialised path.
      if (fl.pairs.on) return fail(SVS_ERR_INVALID, "internal: the 16-query kernels have no pair mode");
      launch_q16(idx, r, p);
      break;
    case BatchRoute::TILED_F32:
      with_bool(fl.state != nullptr, [&](auto fuse) {
        r.tile == 64 ? launch_tiled_bn<64, fuse(), 4>(idx, c, r.nq, p) : launch_tiled_bn<32, fuse(), 4>(idx, c, r.nq, p);
      });
      break;
    case BatchRoute::TILED_EB:
      idx->dtype == SVS_DTYPE_F16 ? launch_tiled_eb<2>(idx, c, r, p) : launch_tiled_eb<1>(idx, c, r, p);
      break;
    case BatchRoute::LOOP:
      if (name) { *name = "gemv"; break; }
      if (fl.state || n_rows != idx->n) return fail(SVS_ERR_INVALID, "internal: single-query kernels have no fused / prefix form");
      launch_record("gemv", n_rows, r.nq);   // (one entry for the per-query loop)
      for (int qi = 0; qi < r.nq; ++qi) {
        const int rc = launch_scores(idx, c, r.single, (const float*)q + (size_t)qi * idx->d, scores + (size_t)qi * sstride, st);
        if (rc != SVS_OK) return rc;
      }
      break;
  }
  return SVS_OK;
}

// run_select's route over n_eff scores: one workgroup sorts them all; beyond SORT_CAP, up to SEL_KMAX results come from
// a histogram window and its candidates (the context's hist / cand scratch), more from a global sort (its keys scratch)
enum class SelectPath { FINAL, WINDOW, SORT };
constexpr SelectPath select_path(int64_t n_eff, int count) {
  return n_eff > SORT_CAP && count <= SEL_KMAX ? SelectPath::WINDOW : (n_eff > SORT_CAP ? SelectPath::SORT : SelectPath::FINAL);
}

// Histogram / candidate scratch of run_select's window path (SelectPath::WINDOW) for nq queries.
int grow_select_scratch(Ctx* c, int nq, hipStream_t st) {
  if ((size_t)nq <= c->hist_cap) return SVS_OK;
  c->hist_cap = 0;
  HIP_TRY(c->hist.release());
  HIP_TRY(c->cand.release());
  int rc;
  if ((rc = c->hist.grow((size_t)nq * SCR_WORDS)) != SVS_OK) return rc;
  if ((rc = c->cand.grow((size_t)nq * CAND_CAP)) != SVS_OK) return rc;
  // zeroed once; select_final_kernel leaves it zeroed after every search
  HIP_TRY(hipMemsetAsync(c->hist, 0, (size_t)nq * SCR_WORDS * sizeof(uint32_t), st));
  c->hist_cap = nq;
  return SVS_OK;
}

// Top-k stage over a materialised score matrix scores[nq][sstride] with n_eff rows.
int run_select(svs_index* idx, Ctx* c, const float* scores, int64_t n_eff, int64_t sstride, int nq, int k,
               int count, float* out_s, int64_t* out_r, hipStream_t st, int64_t row_offset) {
  int rc;
  uint32_t* hist = c->hist;
  uint64_t* cand = c->cand;
  const SelectPath path = select_path(n_eff, count);
  if (path == SelectPath::FINAL) {
    hipLaunchKernelGGL(select_final_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, scores, n_eff, sstride, k, count, 1,
                       (uint32_t*)nullptr, (uint64_t*)nullptr, row_offset, out_s, out_r, (const uint32_t*)nullptr);
  } else if (path == SelectPath::WINDOW) {
    const int64_t per_block = (int64_t)FA_THREADS * SEL_VPT * 4;
    const unsigned blocks = (unsigned)((n_eff + per_block - 1) / per_block);
    hipLaunchKernelGGL(select_window_hist_kernel, dim3(blocks, nq), dim3(FA_THREADS), 0, st, scores, n_eff, sstride, hist);
    hipLaunchKernelGGL(select_window_filter_kernel, dim3(blocks, nq), dim3(FA_THREADS), 0, st, scores, n_eff, sstride,
                       (uint32_t)count, hist, cand);
    hipLaunchKernelGGL(select_final_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, scores, n_eff, sstride, k, count, 0,
                       hist, cand, row_offset, out_s, out_r, (const uint32_t*)nullptr);
  } else {
    const int64_t npad = next_pow2_i64(n_eff);
    if ((rc = c->keys.grow((size_t)nq * (size_t)npad)) != SVS_OK) return rc;
    int gb = (int)std::min<int64_t>((npad + 255) / 256, 4096);
    hipLaunchKernelGGL(keys_build_kernel, dim3(gb, nq), dim3(256), 0, st, scores, n_eff, sstride, npad, c->keys);
    const int64_t chunk = std::min<int64_t>(npad, SORT_CAP);
    hipLaunchKernelGGL(bitonic_local_kernel, dim3((unsigned)(npad / chunk), nq), dim3(SORT_THREADS), 0, st, c->keys, npad, 0, 1);
    for (int64_t size = 2 * (int64_t)SORT_CAP; size <= npad; size <<= 1) {
      for (int64_t stride = size >> 1; stride >= SORT_CAP; stride >>= 1) {
        int g2 = (int)std::min<int64_t>(((npad >> 1) + 255) / 256, 8192);
        hipLaunchKernelGGL(bitonic_global_kernel, dim3(g2, nq), dim3(256), 0, st, c->keys, npad, size, stride);
      }
      hipLaunchKernelGGL(bitonic_local_kernel, dim3((unsigned)(npad / chunk), nq), dim3(SORT_THREADS), 0, st, c->keys, npad, size, 0);
    }
    int ge = std::min((k + 255) / 256, 1024);
    hipLaunchKernelGGL(keys_emit_kernel, dim3(ge, nq), dim3(256), 0, st, c->keys, npad, k, count,
                       row_offset, out_s, out_r);
  }
  return SVS_OK;
}

// ---- screened single-query search over an f32 corpus (screen.h) --------------------------------
// Rows below which a screened query is not ahead of the plain f32 pass by more than the run-to-run spread (one more
// launch, the gather; measured with tools/screen_threshold.py, table in DESIGN.md): at 32,768 rows it is 15-22 % ahead
// for rows of 1536-4096 floats and level (1.02 x) for rows of 512, which are ahead from 65,536 (0.87 x).
// svs_index_set_variant(12) screens whatever n, 11 never.
inline int64_t screen_min_rows(int ld) { return ld <= 512 ? 65536 : 32768; }

constexpr int rescore_u(int nstep) { return nstep <= 4 ? 4 : (nstep <= 8 ? 2 : 1); }
template <int NSTEP>
constexpr KernelName kRescoreName = kernel_name("rescore_f32_kernel", NSTEP, rescore_u(NSTEP));

bool screen_ready(const svs_index* idx) {
  return idx->dtype == SVS_DTYPE_F32 && idx->shadow && idx->scr_dev && idx->scr_host && idx->screen_mode.load() == 1 &&
         !idx->shadow_bad.load() && !idx->scr_paused.load();
}

// Fallbacks (exact, but the screen pass on top of the f32 pass) dominating the recent queries: stop screening until the
// next ingest.  The counters are written by the re-score kernel into pinned memory; read here without synchronising.
void screen_review(svs_index* idx) {
  uint64_t s_tot = 0, f_tot = 0;
  const volatile uint32_t* h = idx->scr_host;
  for (int i = 0; i < svs_index::kSlots; ++i) {
    s_tot += h[i * SCREEN_SLOT_WORDS];
    f_tot += h[i * SCREEN_SLOT_WORDS + 1];
  }
  const uint64_t ds = s_tot - idx->scr_base_s.load(), df = f_tot - idx->scr_base_f.load();
  if (ds + df < 32) return;
  if (df > ds) {
    idx->scr_paused.store(true);
    idx->geo_epoch.fetch_add(1);
  }
  idx->scr_base_s.store(s_tot);
  idx->scr_base_f.store(f_tot);
}

thread_local const svs_index* g_screen_idx;   // svs_internal_screen_stats: the calling thread's last screened search
thread_local int g_screen_slot;

// steps 2-5 (step 1, approximate scores from the half shadow, is the route single_route(idx, variant, true)): histogram, filter with margin, exact re-score of the candidates, final top-k
int run_select_screened(svs_index* idx, Ctx* c, const float* q_padded, int k, int count, float* out_s, int64_t* out_r,
                        hipStream_t st) {
  const int64_t n = idx->n, sstride = score_stride(n);
  const int64_t per_block = (int64_t)FA_THREADS * SEL_VPT * 4;
  const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
  uint32_t* cnt_dev = idx->scr_dev + sizeof(ScreenStats) / 4 + (size_t)c->slot * SCREEN_SLOT_WORDS;
  uint32_t* slot_host = idx->scr_host + (size_t)c->slot * SCREEN_SLOT_WORDS;
  g_screen_idx = idx;
  g_screen_slot = c->slot;
  hipLaunchKernelGGL(select_window_hist_kernel, dim3(blocks, 1), dim3(FA_THREADS), 0, st, (const float*)c->scores, n, sstride, c->hist);
  hipLaunchKernelGGL(screen_filter_kernel, dim3(blocks), dim3(FA_THREADS), 0, st, (const float*)c->scores, n, (uint32_t)count,
                     c->hist, c->cand, q_padded, idx->ld, (const ScreenStats*)idx->scr_dev, slot_host);
  const uint32_t* dead_bits = dead_bits_of(idx);
  const int rblocks = idx->cu_count * 4;
  switch (idx->ld / 256) {
#define SVS_RESCORE_CASE(N)                                                                                          \
  case N:                                                                                                            \
    launch_record(kRescoreName<N>.s, n, 1);                                                                          \
    hipLaunchKernelGGL((rescore_f32_kernel<N, rescore_u(N)>), dim3(rblocks), dim3(256), 0, st, (const v4f*)idx->rows, \
                       (const v4f*)q_padded, c->scores, n, (const uint32_t*)c->hist, c->cand, dead_bits, cnt_dev,     \
                       slot_host);                                                                                   \
    break;
    SVS_RESCORE_CASE(2) SVS_RESCORE_CASE(4) SVS_RESCORE_CASE(6) SVS_RESCORE_CASE(8) SVS_RESCORE_CASE(10)
    SVS_RESCORE_CASE(12) SVS_RESCORE_CASE(14) SVS_RESCORE_CASE(16)
#undef SVS_RESCORE_CASE
    default: return fail(SVS_ERR_INVALID, "internal: no re-score kernel for ld %d", idx->ld);
  }
  hipLaunchKernelGGL(select_final_kernel, dim3(1), dim3(FINAL_THREADS), 0, st, (const float*)c->scores, n, sstride, k, count, 0,
                     c->hist, c->cand, idx->row_offset, out_s, out_r, (const uint32_t*)nullptr);
  return SVS_OK;
}

// ---- filtered search: scores of nq queries over a row list (gather.h) ---------------------------
template <int DT, int T, int NC, int U, int G>
constexpr KernelName kGatherName = kernel_name("gather_scores_kernel", DT, T, NC, U, G);

template <int DT, int T, int NC, int U>
void launch_gather_geo(const svs_index* idx, const void* q, const float* q_scales, int nq, const uint32_t* list, int64_t m,
                       float* scores, int64_t sstride, int ld16, hipStream_t st) {
  constexpr int WPB = gather_wpb(NC);
  constexpr int64_t per_block = (int64_t)(64 / T) * U * WPB;
  const unsigned blocks = (unsigned)((m + per_block - 1) / per_block);
  if (nq == 1) {
    launch_record(kGatherName<DT, T, NC, U, 1>.s, m, nq);
    hipLaunchKernelGGL((gather_scores_kernel<DT, T, NC, U, 1>), dim3(blocks, 1), dim3(WPB * 64), 0, st,
                       (const u32x4*)idx->rows, ld16, list, m, (const u32x4*)q, nq, idx->row_scales, q_scales, scores, sstride);
  } else {
    launch_record(kGatherName<DT, T, NC, U, GATHER_G>.s, m, nq);
    const size_t lds = (size_t)std::min(nq, GATHER_G) * ld16 * 16;
    hipLaunchKernelGGL((gather_scores_kernel<DT, T, NC, U, GATHER_G>), dim3(blocks, (nq + GATHER_G - 1) / GATHER_G),
                       dim3(WPB * 64), lds, st, (const u32x4*)idx->rows, ld16, list, m, (const u32x4*)q, nq,
                       idx->row_scales, q_scales, scores, sstride);
  }
}

// q: nq staged queries ([nq][ld] in the corpus dtype, zero padded); list: m local rows on the device
template <int DT>
int launch_gather_dt(const svs_index* idx, const void* q, const float* q_scales, int nq, const uint32_t* list, int64_t m,
                     float* scores, int64_t sstride, hipStream_t st) {
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  const bool ok = for_row_geometry(ld16, [&](auto t, auto nc) {
    launch_gather_geo<DT, t(), nc(), gather_u(nc())>(idx, q, q_scales, nq, list, m, scores, sstride, ld16, st);
  });
  if (ok) return SVS_OK;
  return fail(SVS_ERR_UNSUPPORTED, "svs_index_search_rows: rows of %d bytes; the gather kernel takes rows of up to 16 KiB",
              ld16 * 16);
}

// nq f32 queries on the device as the gather kernels read them: [nq][ld] in the corpus dtype, zero padded, in the
// context's staging buffers.  *q_scales: their scales (fp8), else null.
int stage_gather_queries(const svs_index* idx, Ctx* c, const float* q_dev, int nq, const void** q, const float** q_scales, hipStream_t st) {
  int rc;
  *q_scales = nullptr;
  if (idx->dtype == SVS_DTYPE_F32) {
    const float* qs = nullptr;
    if ((rc = stage_queries_f32(idx, c, q_dev, nq, nq, &qs, st)) != SVS_OK) return rc;
    *q = qs;
  } else if (idx->dtype == SVS_DTYPE_F16) {
    if ((rc = stage_queries_f16(idx, c, q_dev, nq, nq, st)) != SVS_OK) return rc;
    *q = c->qh.p;
  } else {
    if ((rc = stage_queries_fp8(idx, c, q_dev, nq, nq, false, st)) != SVS_OK) return rc;
    *q = c->q8.p;
    *q_scales = c->q8s.p;
  }
  return SVS_OK;
}

// f(Int<DT>): the corpus dtype as the template argument of the kernels that read stored rows (0 f32, 1 f16, 2 fp8)
template <class F>
auto for_store_dtype(const svs_index* idx, F&& f) {
  return idx->dtype == SVS_DTYPE_F32 ? f(Int<0>{}) : (idx->dtype == SVS_DTYPE_F16 ? f(Int<1>{}) : f(Int<2>{}));
}

// Stages queries [q0, q0 + nq) of the call (f32 in c->q_dev) in the corpus dtype and scores them over the list.
int launch_gather(const svs_index* idx, Ctx* c, const float* q_dev, int nq, const uint32_t* list, int64_t m, float* scores,
                  int64_t sstride, hipStream_t st) {
  const void* q = nullptr;
  const float* qs = nullptr;
  const int rc = stage_gather_queries(idx, c, q_dev, nq, &q, &qs, st);
  if (rc != SVS_OK) return rc;
  return for_store_dtype(idx, [&](auto dt) { return launch_gather_dt<dt()>(idx, q, qs, nq, list, m, scores, sstride, st); });
}

// Top `count` of nq queries (f32 on the device) over a device row list: m local rows, ascending.  The context's score
// matrix and select scratch are the caller's to size.  out_r receives POSITIONS in the list: list_positions_to_rows.
int enqueue_list_search(svs_index* idx, Ctx* c, const float* q_dev, int nq, const uint32_t* list, int64_t m, int count, float* out_s,
                        int64_t* out_r, hipStream_t st) {
  const int64_t sstride = score_stride(m);
  const int rc = launch_gather(idx, c, q_dev, nq, list, m, c->scores, sstride, st);
  return rc != SVS_OK ? rc : run_select(idx, c, c->scores, m, sstride, nq, count, count, out_s, out_r, st, 0);
}

// The call's nq queries (f32 in c->q_dev, d columns) over one device list, sized here: query chunks whose score matrix
// (and, for k > SEL_KMAX over more than SORT_CAP rows, sort keys) stays <= 2 GiB.  out_s / out_r: [nq][count].
int search_list_chunked(svs_index* idx, Ctx* c, int nq, int d, const uint32_t* list_dev, int64_t m, int count, float* out_s,
                        int64_t* out_r, hipStream_t st) {
  const int64_t sstride = score_stride(m);
  int64_t per_q = 4 * sstride;
  const SelectPath sel = select_path(m, count);
  if (sel == SelectPath::SORT) per_q += 8 * next_pow2_i64(m);
  const int qc = (int)std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)2 << 30) / per_q));
  int rc;
  if ((rc = c->scores.grow((size_t)qc * (size_t)sstride)) != SVS_OK) return rc;
  if (sel == SelectPath::WINDOW && (rc = grow_select_scratch(c, qc, st)) != SVS_OK) return rc;
  for (int q0 = 0; q0 < nq; q0 += qc) {
    const int nc = std::min(qc, nq - q0);
    if ((rc = enqueue_list_search(idx, c, c->q_dev + (size_t)q0 * d, nc, list_dev, m, count, out_s + (size_t)q0 * count,
                                  out_r + (size_t)q0 * count, st)) != SVS_OK)
      return rc;
  }
  return SVS_OK;
}

// ... and, once they have arrived in pinned memory, the positions -> global rows, in place.  S: the list on the host;
// seg: the segment it belongs to (the error's text), -1 for the one list of svs_index_search_rows.
int list_positions_to_rows(int64_t* r, size_t cnt, const uint32_t* S, int64_t m, int64_t lo, int seg) {
  for (size_t i = 0; i < cnt; ++i) {
    const int64_t p = r[i];
    if (p < 0 || p >= m)
      return seg < 0 ? fail(SVS_ERR_DEVICE, "search_rows: position %lld outside the %lld listed rows", (long long)p, (long long)m)
                     : fail(SVS_ERR_DEVICE, "search_segments: position %lld outside the %lld listed rows of segment %d", (long long)p,
                            (long long)m, seg);
    r[i] = (int64_t)S[p] + lo;
  }
  return SVS_OK;
}

// ---- segmented filtered search: the small segments of a call in two launches (segments.h) -----------
template <int DT, int T, int NC, int U>
constexpr KernelName kGatherSegName = kernel_name("gather_segments_kernel", DT, T, NC, U);

// Rows a wave of the gather kernels takes on this index (0: rows longer than 16 KiB, which they do not take)
int gather_rows_per_wave(const svs_index* idx) {
  int w = 0;
  for_row_geometry((int)((size_t)idx->ld * elem_bytes(idx) / 16), [&](auto t, auto nc) { w = 64 / t() * gather_u(nc()); });
  return w;
}

// q: the call's staged queries ([nq][ld] in the corpus dtype); list, tiles: on the device; total_rows, nseg: what the
// tiles cover (the launch record)
template <int DT>
void launch_gather_segments_dt(const svs_index* idx, const void* q, const float* q_scales, const uint32_t* list, const SegTile* tiles,
                               int64_t ntiles, int64_t total_rows, int nseg, float* scores, hipStream_t st) {
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  for_row_geometry(ld16, [&](auto t, auto nc) {
    constexpr int T = t(), NC = nc(), U = gather_u(NC), WPB = gather_wpb(NC);
    launch_record(kGatherSegName<DT, T, NC, U>.s, total_rows, nseg);
    hipLaunchKernelGGL((gather_segments_kernel<DT, T, NC, U>), dim3((unsigned)((ntiles + WPB - 1) / WPB)), dim3(WPB * 64), 0, st,
                       (const u32x4*)idx->rows, ld16, list, tiles, ntiles, (const u32x4*)q, idx->row_scales, q_scales, scores);
  });
}

// Stages the call's nq queries (f32 in q_dev) in the corpus dtype, once, and scores every tile
int launch_gather_segments(const svs_index* idx, Ctx* c, const float* q_dev, int nq, const uint32_t* list, const SegTile* tiles,
                           int64_t ntiles, int64_t total_rows, int nseg, float* scores, hipStream_t st) {
  const void* q = nullptr;
  const float* qs = nullptr;
  const int rc = stage_gather_queries(idx, c, q_dev, nq, &q, &qs, st);
  if (rc != SVS_OK) return rc;
  for_store_dtype(idx, [&](auto dt) { launch_gather_segments_dt<dt()>(idx, q, qs, list, tiles, ntiles, total_rows, nseg, scores, st); });
  return SVS_OK;
}

// One batch through a route of its own -- decided, staged, launched (the pair paths, chunk by chunk).  variant: the call's
int score_batch(const svs_index* idx, Ctx* c, int variant, const float* q_dev, int nq, int64_t n_rows, float* scores, int64_t sstride,
                FuseLaunch fl, hipStream_t st) {
  const BatchRoute r = batch_route(idx, variant, nq);
  const void* q = nullptr;
  const int rc = stage_batch(idx, c, r, q_dev, st, &q);
  return rc != SVS_OK ? rc : launch_batch(idx, c, r, q, n_rows, scores, sstride, fl, st);
}

// rows whose exact k-th best seeds the fused epilogue's thresholds: about k * n / prefix
// candidates per query survive, so the prefix grows with n (n/64 -> ~64 k survivors)
constexpr int64_t FUSE_PREFIX_MIN = 16384;
constexpr int64_t PFX_BLOCK = 256;   // rows per block of the threshold sample (one row tile of the MFMA kernels)
inline int64_t fuse_prefix_rows(int64_t n) {
  const int64_t p = std::max<int64_t>(FUSE_PREFIX_MIN, n / std::max<int64_t>(g_tune_prefix_div.load(), 1));
  return (p + PFX_BLOCK - 1) / PFX_BLOCK * PFX_BLOCK;
}

// The rows the fused path takes its thresholds from.  Rounds 1-3 used the FIRST n / 64 rows: a corpus whose first rows
// are unlike the rest (sorted by similarity to what is asked, or drifting) then gives thresholds that cut nothing, every
// candidate list overflows and the batch falls back to the materialised path.  Any n_mat rows of the corpus give a valid
// bound (the k-th best of a subset is never above the k-th best of the whole), so the sample is taken in blocks of 256
// rows EVERY n / (n_mat / 256) rows -- one strided device-to-device copy into a contiguous image the batched kernels run
// over unchanged -- and is as good a picture of a sorted corpus as of a shuffled one.  1.6 % more HBM; rebuilt (20 us at
// 1M x 1536 f16) when rows were appended.  Rebuilding frees nothing a kernel may still read: the row count only changes
// under the exclusive geometry lock, i.e. after every fused search has drained (the host entry synchronises).
int prefix_image(svs_index* idx, int64_t n_mat, hipStream_t st) {
  std::lock_guard<std::mutex> lk(idx->pfx_mu);
  if (idx->pfx_n == idx->n && idx->pfx_nmat == n_mat && idx->pfx_src == idx->rows) return SVS_OK;
  const int64_t nblk = n_mat / PFX_BLOCK, stride = idx->n / nblk;   // (stride >= PFX_BLOCK: n_mat <= n)
  const size_t rowb = (size_t)idx->ld * elem_bytes(idx);
  if ((size_t)n_mat > idx->pfx_cap) {
    if (idx->pfx_rows) HIP_TRY(hipFree(idx->pfx_rows));
    if (idx->pfx_scales) HIP_TRY(hipFree(idx->pfx_scales));
    idx->pfx_rows = nullptr; idx->pfx_scales = nullptr; idx->pfx_cap = 0; idx->pfx_n = -1;
    if (hipMalloc(&idx->pfx_rows, (size_t)n_mat * rowb) != hipSuccess)
      return fail(SVS_ERR_NOMEM, "out of HBM for the %lld-row threshold sample", (long long)n_mat);
    if (idx->row_scales && hipMalloc((void**)&idx->pfx_scales, (size_t)n_mat * sizeof(float)) != hipSuccess)
      return fail(SVS_ERR_NOMEM, "out of HBM for the threshold sample's row scales");
    idx->pfx_cap = (size_t)n_mat;
  }
  HIP_TRY(hipMemcpy2DAsync(idx->pfx_rows, (size_t)PFX_BLOCK * rowb, idx->rows, (size_t)stride * rowb, (size_t)PFX_BLOCK * rowb,
                           (size_t)nblk, hipMemcpyDeviceToDevice, st));
  if (idx->row_scales)
    HIP_TRY(hipMemcpy2DAsync(idx->pfx_scales, (size_t)PFX_BLOCK * sizeof(float), idx->row_scales, (size_t)stride * sizeof(float),
                             (size_t)PFX_BLOCK * sizeof(float), (size_t)nblk, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));   // (searches on other streams use the image as soon as the lock is gone)
  idx->pfx_n = idx->n; idx->pfx_nmat = n_mat; idx->pfx_stride = stride; idx->pfx_src = idx->rows;
  return SVS_OK;
}

// One search, enqueued in three steps (the host API sizes scratch and starts the timing events BEFORE it stages
// the queries, so that everything the device does for a call sits between the call's events):
//   plan_search     decisions (materialised / fused, prefix size), scratch, the timing start event
//   enqueue_prefix  fused only: the queries staged in the corpus dtype, their scores over the prefix rows, their
//                   thresholds (exact k-th best of the prefix)
//   enqueue_main    fused: the whole-corpus pass with the threshold epilogue + final select; otherwise the
//                   materialised score stage + top-k stage
// (Round 4 built and measured the prefix step PER QUERY TILE -- tile t's staging, prefix GEMM and thresholds enqueued
//  behind its DMA while tile t + 1 was still being copied: configs[2] 3.26 ms per call against 3.04.  One query tile's
//  prefix GEMM is 64 output tiles, a quarter of the CUs, and takes as long as the whole batch's 256; and every
//  copy -> kernel -> copy alternation on the stream is a hand-over between the DMA engine and the compute queue.)
struct SearchPlan {
  int nq = 0, k = 0, count = 0;
  bool path_a = false, fused = false, kth = false, timed = false;
  bool screen = false;   // one query over an f32 index with a valid half shadow: screen.h
  int64_t n_mat = 0, sstride = 0;
  SingleRoute route{};               // nq == 1: the score kernel, under the variant the plan was made with (single_route)
  BatchRoute batch{};                // nq >= 2: family, query tile and staging of every pass of the call (batch_route)
  const void* q_staged = nullptr;    // ... and the queries as its kernels read them: null until stage_batch (or search_host,
                                     // chunk by chunk) has staged them, in front of the call's first pass
  const float* q_padded = nullptr;   // screened search: the query as launch_scores staged it (the re-score reads it)
  EvTriple ev{};
  hipEvent_t pass_stop = nullptr;    // run-ahead pipeline, one query: the event the LAST kernel of the score half is to carry (launch_tail)
  bool pass_bound = false;           // ... and it does (enqueue_score_half): nothing was recorded for it
  // run-ahead pipeline, shareable search (enqueue_ahead): the claim kernel's launch in front of the pass
  const AheadPipe* share = nullptr;
  uint64_t share_num = 0, share_reach = 0, share_epoch = 0;
  bool share_thin = false;           // ... and the pass on a thin grid
};

int plan_search(svs_index* idx, Ctx* c, int nq, int k, int count, hipStream_t st, bool allow_fused, int variant, SearchPlan* p) {
  const int64_t n = idx->n;
  int rc;
  if ((rc = staging_wait(idx)) != SVS_OK) return rc;
  p->nq = nq; p->k = k; p->count = count;
  p->path_a = k > 0 && select_path(n, count) == SelectPath::WINDOW;
  // Fused top-k epilogue (no score matrix) for the batched kernels; a query whose
  // candidate list overflows comes back marked and is re-run by the caller.  The prefix
  // pass costs ~60 us whatever the batch: measured break-even is 16 queries (f32: 13.2 k vs
  // 12.7 k queries/s at 16, 6.4 k vs 6.5 k at 8; f16 at 32: 49 k vs 41 k; fp8 at 32: 77 k vs 64 k).
  if (nq != 1) p->batch = batch_route(idx, variant, nq);
  p->fused = allow_fused && p->path_a && p->batch.family != BatchRoute::LOOP && nq >= 16 &&
             n >= 8 * FUSE_PREFIX_MIN && (int64_t)n < ((int64_t)1 << 32) &&
             count <= 256 && variant != VARIANT_NO_FUSION;
  p->screen = nq == 1 && p->path_a && screen_ready(idx) &&
              variant != VARIANT_SCREEN_OFF && (variant == VARIANT_SCREEN_FORCE || (variant == VARIANT_DEFAULT && n >= screen_min_rows(idx->ld)));
  if (p->screen) {
    screen_review(idx);
    p->screen = !idx->scr_paused.load();
  }
  if (nq == 1) p->route = single_route(idx, variant, p->screen);
  p->n_mat = p->fused ? fuse_prefix_rows(n) : n;       // rows of the materialised score matrix
  p->sstride = score_stride(p->n_mat);           // float4-aligned score vectors
  // thresholds: many queries over a short prefix -> one k-th-value kernel (47 vs 62 us at 1024 x 16,384);
  // otherwise the ordinary three-launch top-k, whose kernels spread one query over many workgroups
  // (16 queries: 20 vs 33 us; 256 x 156,250 rows: 119 vs 284 us).
  p->kth = p->fused && nq >= 256 && p->n_mat <= 32768;
  if ((rc = c->scores.grow((size_t)nq * (size_t)p->sstride)) != SVS_OK) return rc;
  if (p->path_a && (rc = grow_select_scratch(c, nq, st)) != SVS_OK) return rc;
  if (p->fused) {
    if ((rc = c->pref_s.grow((size_t)nq * (p->kth ? 1 : count))) != SVS_OK) return rc;
    if (!p->kth && (rc = c->pref_r.grow((size_t)nq * count)) != SVS_OK) return rc;
  }
  const int tevery = idx->timing.load();
  p->timed = tevery > 0 && (idx->timing_seq.fetch_add(1) % (uint32_t)tevery) == 0;
  if (p->timed) {
    HIP_TRY(hipEventCreate(&p->ev.e0));
    HIP_TRY(hipEventCreate(&p->ev.e1));
    HIP_TRY(hipEventCreate(&p->ev.e2));
    HIP_TRY(hipEventRecord(p->ev.e0, st));
  }
  return SVS_OK;
}

int enqueue_prefix(svs_index* idx, Ctx* c, SearchPlan& p, const float* q_dev, hipStream_t st) {
  if (!p.fused) return SVS_OK;
  int rc;
  const int nq = p.nq, count = p.count;
  FuseLaunch sample{};
  int64_t blk_stride = 0;
  if (g_tune_spread.load()) {
    if ((rc = prefix_image(idx, p.n_mat, st)) != SVS_OK) return rc;
    sample.rows = idx->pfx_rows;
    sample.row_scales = idx->pfx_scales;
    blk_stride = idx->pfx_stride;
  }
  if (!p.q_staged && (rc = stage_batch(idx, c, p.batch, q_dev, st, &p.q_staged)) != SVS_OK) return rc;
  if ((rc = launch_batch(idx, c, p.batch, p.q_staged, p.n_mat, c->scores, p.sstride, sample, st)) != SVS_OK) return rc;
  if (!idx->dead_list.empty())   // thresholds must come from LIVE rows: masked sample rows -> -inf (rows outside the sample are skipped)
    hipLaunchKernelGGL(mask_dead_rows_kernel, dim3(64), dim3(256), 0, st, c->scores, p.sstride, nq, idx->dead_dev,
                       (int64_t)idx->dead_list.size(), p.n_mat, blk_stride);
  if (p.kth)
    hipLaunchKernelGGL(prefix_kth_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, (const float*)c->scores, p.n_mat, p.sstride, count, c->pref_s);
  else if ((rc = run_select(idx, c, c->scores, p.n_mat, p.sstride, nq, count, count, c->pref_s, c->pref_r, st, idx->row_offset)) != SVS_OK)
    return rc;
  return SVS_OK;
}

// enqueue_main in two halves, so that svs_index_search_device_ahead can put them on two streams: everything up to and
// including the `e1` timing event (query padding and staging, the screen pass or the score launch, the tombstone
// mask), then the selection.  Both take the same plan; q_padded carries the staged query of a screened search across.
int enqueue_score_half(svs_index* idx, Ctx* c, SearchPlan& p, const float* q_dev, hipStream_t st) {
  const int64_t n = idx->n;
  const int nq = p.nq, count = p.count;
  int rc;
  EvTriple& ev = p.ev;
  if (p.fused) {
    // the whole corpus, keeping only scores >= threshold (the queries are staged: enqueue_prefix)
    FuseLaunch fl{c->hist, c->cand, p.kth ? c->pref_s : c->pref_s + (count - 1), p.kth ? 1 : count};
    if (p.timed) {
      HIP_TRY(hipEventCreate(&ev.d0));
      HIP_TRY(hipEventCreate(&ev.d1));
      HIP_TRY(hipEventRecord(ev.d0, st));
    }
    if ((rc = launch_batch(idx, c, p.batch, p.q_staged, n, nullptr, 0, fl, st)) != SVS_OK) return rc;
    if (p.timed) HIP_TRY(hipEventRecord(ev.d1, st));
    if (p.timed) HIP_TRY(hipEventRecord(ev.e1, st));
    return SVS_OK;
  }
  // (the half's LAST kernel is handed p.pass_stop: the mask when there are tombstones, else the score kernel)
  const bool masked = !idx->dead_list.empty(), carry = p.pass_stop && nq == 1;
  if (nq == 1) {
    PassOpts o;
    if (carry && !masked) o.stop = p.pass_stop;
    if (p.share) {   // what this pass serves is decided here, on the pass stream, and nowhere else (pass_share.h)
      const AheadPipe* sp = p.share;
      hipLaunchKernelGGL(pass_claim_kernel, dim3(1), dim3(64), 0, st, (const MailEntry*)sp->mailbox, sp->share_dev, sp->share_mirror(),
                         p.share_num, p.share_reach, sp->share_limit, (const v4f*)q_dev, c->scores.p, (uint64_t)(uintptr_t)half_rows_of(idx, p.route),
                         (uint64_t)n, p.share_epoch, (uint64_t)idx->ld, p.share_thin ? 1 : 0);
      o = PassOpts{o.stop, &sp->share_dev->plan, sp->share_limit, p.share_thin};
    }
    if (!p.screen) launch_record("gemv", n, 1);   // (as launch_batch announces its per-query loop)
    rc = launch_scores(idx, c, p.route, q_dev, c->scores, st, o, &p.q_padded);
  } else if (p.q_staged || (rc = stage_batch(idx, c, p.batch, q_dev, st, &p.q_staged)) == SVS_OK) {
    rc = launch_batch(idx, c, p.batch, p.q_staged, n, c->scores, p.sstride, FuseLaunch{}, st);
  }
  if (rc != SVS_OK) return rc;
  if (masked)   // tombstoned rows can never be returned
    launch_tail(carry ? p.pass_stop : nullptr, mask_dead_rows_kernel, dim3(64), dim3(256), 0, st, c->scores.p, p.sstride, nq, idx->dead_dev.p,
                (int64_t)idx->dead_list.size(), n, (int64_t)0);
  p.pass_bound = carry;
  if (p.timed && !(p.pass_bound && p.pass_stop == ev.e1)) HIP_TRY(hipEventRecord(ev.e1, st));
  return SVS_OK;
}

int enqueue_select_half(svs_index* idx, Ctx* c, SearchPlan& p, float* out_s, int64_t* out_r, hipStream_t st) {
  const int64_t n = idx->n;
  const int nq = p.nq, k = p.k, count = p.count;
  int rc;
  EvTriple& ev = p.ev;
  if (p.fused) {
    hipLaunchKernelGGL(select_final_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, (const float*)nullptr, n, (int64_t)0, k, count, 3,
                       c->hist, c->cand, idx->row_offset, out_s, out_r,
                       dead_bits_of(idx));
  } else if (p.screen) {   // (stage_ms.score is the screen pass; the exact re-score of the candidates counts as select)
    if ((rc = run_select_screened(idx, c, p.q_padded, k, count, out_s, out_r, st)) != SVS_OK) return rc;
  } else if (k > 0 && (rc = run_select(idx, c, c->scores, n, p.sstride, nq, k, count, out_s, out_r, st, idx->row_offset)) != SVS_OK) {
    return rc;
  }
  HIP_TRY(hipGetLastError());
  if (p.timed) {
    HIP_TRY(hipEventRecord(ev.e2, st));
    std::lock_guard<std::mutex> lk(idx->mu);
    idx->evs.push_back(ev);
  }
  return SVS_OK;
}

int enqueue_main(svs_index* idx, Ctx* c, SearchPlan& p, const float* q_dev, float* out_s, int64_t* out_r, hipStream_t st) {
  int rc = enqueue_score_half(idx, c, p, q_dev, st);
  if (rc != SVS_OK) return rc;
  return enqueue_select_half(idx, c, p, out_s, out_r, st);
}

int enqueue_search(svs_index* idx, Ctx* c, const float* q_dev, int nq, int k, int count,
                   float* out_s, int64_t* out_r, hipStream_t st, bool allow_fused = false) {
  SearchPlan p;
  int rc;
  if ((rc = plan_search(idx, c, nq, k, count, st, allow_fused, idx->variant.load(), &p)) != SVS_OK) return rc;
  if ((rc = enqueue_prefix(idx, c, p, q_dev, st)) != SVS_OK) return rc;
  return enqueue_main(idx, c, p, q_dev, out_s, out_r, st);
}

// Holds one reference for the duration of a call.  Declared BEFORE the geometry lock in every
// entry point: locals unwind in reverse order, so the lock is dropped first and only then the
// reference -- if a concurrent svs_index_release() made ours the last one, index_destroy() must
// not run while this call still holds idx->rw.
struct RefGuard {
  svs_index* i;
  explicit RefGuard(svs_index* idx) : i(idx) { i->refs.fetch_add(1); }
  ~RefGuard() { svs_index_release(i); }
  RefGuard(const RefGuard&) = delete;
  RefGuard& operator=(const RefGuard&) = delete;
};

// Hands an acquired search context back on scope exit.
struct CtxGuard {
  svs_index* i;
  Ctx* c;
  ~CtxGuard() { ctx_release(i, c); }
};

// A host-driven call's hold on a search context and the context's own stream.  Declared after validation, under the
// entry's RefGuard and geometry lock, and opened at once.  What it guarantees: no context returns to the free list with
// work in flight -- whatever the call enqueued has drained when the frame goes, on EVERY exit.  A context taken from the
// list with async_pending false is therefore idle, and the next host call may memcpy into its pinned buffers at once.
struct HostCall {
  svs_index* idx;
  Ctx* c = nullptr;
  bool busy = false;   // enqueued since the last wait
  explicit HostCall(svs_index* i) : idx(i) {}
  HostCall(const HostCall&) = delete;
  ~HostCall() {
    if (c && busy) (void)hipStreamSynchronize(c->stream);
    if (c) ctx_release(idx, c);
  }
  int open() {
    HIP_TRY(hipSetDevice(idx->device));
    const int rc = staging_wait(idx);
    return rc != SVS_OK ? rc : ctx_acquire(idx, nullptr, true, &c);
  }
  // The stream to enqueue on.  Asking for it marks the call as having work in flight: an exit before that pays no
  // synchronise, one after it drains -- so ask again for what is enqueued behind a wait().
  hipStream_t stream() { busy = true; return c->stream; }
  // The launches so far were accepted ("<entry> launch: ..." / "<entry> re-run: ..."); a refused one drains the stream.
  int launched(const char* entry, bool rerun = false) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SVS_OK;
    (void)wait();
    return fail(SVS_ERR_DEVICE, rerun ? "%s re-run: %s" : "%s launch: %s", entry, hipGetErrorString(e));
  }
  int wait() {
    busy = false;   // (a stream whose wait failed has nothing left to wait for either)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SVS_OK;
  }
  int close(const char* entry, bool rerun = false) { const int rc = launched(entry, rerun); return rc != SVS_OK ? rc : wait(); }
};

// ---- pairwise (document_top_pairwise_scores, src/svs/kb.py:1642-1671) -----------------------
// rows [r0, r0 + nrows) of the corpus as f32 queries (what the index holds), [nrows][d]
int dequant_rows_to(svs_index* idx, int64_t r0, int64_t nrows, float* out, hipStream_t st) {
  if (idx->dtype == SVS_DTYPE_F32)
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)idx->d * sizeof(float), (const float*)idx->rows + r0 * idx->ld, (size_t)idx->ld * sizeof(float),
                             (size_t)idx->d * sizeof(float), (size_t)nrows, hipMemcpyDeviceToDevice, st));
  else if (idx->dtype == SVS_DTYPE_F16)
    hipLaunchKernelGGL(dequant_rows_f16_kernel, dim3(2048), dim3(256), 0, st, (const _Float16*)idx->rows, r0, nrows, idx->d, idx->ld, out);
  else
    hipLaunchKernelGGL(dequant_rows_fp8_kernel, dim3(2048), dim3(256), 0, st, (const uint8_t*)idx->rows, idx->row_scales, r0, nrows,
                       idx->d, idx->ld, out);
  return SVS_OK;
}

// Top `count` pairs among rows [0, ns) (ns * ns_padded <= 2^32): S = M M^T materialised, strict upper
// triangle, the ordinary top-k stage over the flattened matrix (flat index i * np + j reproduces the
// reference's tie order).  Results (scores, flat indices) stay on the device.
int pairs_block_device(svs_index* idx, Ctx* c, int variant, int64_t ns, int count, float* S, float* qbuf, float* d_s, int64_t* d_r, hipStream_t st) {
  const int64_t np = score_stride(ns);
  int rc;
  const int chunk = 1024;
  for (int64_t q0 = 0; q0 < ns; q0 += chunk) {
    const int nq = (int)std::min<int64_t>(chunk, ns - q0);
    if ((rc = dequant_rows_to(idx, q0, nq, qbuf, st)) != SVS_OK) return rc;
    if ((rc = score_batch(idx, c, variant, qbuf, nq, ns, S + q0 * np, np, FuseLaunch{}, st)) != SVS_OK) return rc;
  }
  hipLaunchKernelGGL(mask_upper_triangle_kernel, dim3(4096), dim3(256), 0, st, S, ns, np);
  if (!idx->dead_list.empty())
    hipLaunchKernelGGL(mask_dead_pairs_kernel, dim3(1024), dim3(256), 0, st, S, ns, np, idx->dead_dev, (int64_t)idx->dead_list.size());
  const int64_t flat = ns * np;
  if (select_path(flat, count) == SelectPath::WINDOW && (rc = grow_select_scratch(c, 1, st)) != SVS_OK) return rc;
  if ((rc = run_select(idx, c, S, flat, flat, 1, count, count, d_s, d_r, st, /*row_offset=*/0)) != SVS_OK) return rc;
  HIP_TRY(hipGetLastError());
  return SVS_OK;
}

struct DevTmp {   // frees on scope exit
  std::vector<void*> p;
  template <class T> hipError_t alloc(T** out, size_t bytes) {
    hipError_t e = hipMalloc((void**)out, bytes);
    if (e == hipSuccess) p.push_back((void*)*out);
    return e;
  }
  ~DevTmp() { for (void* q : p) (void)hipFree(q); }
};

int top_pairs_materialised(svs_index* idx, HostCall& fr, int variant, int64_t n, int count, float* out_scores, int64_t* out_i, int64_t* out_j) {
  const int64_t np = score_stride(n);
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  DevTmp tmp;
  float *qbuf = nullptr, *S = nullptr, *d_s = nullptr;
  int64_t* d_r = nullptr;
  HIP_TRY(tmp.alloc(&qbuf, (size_t)1024 * idx->d * sizeof(float)));
  HIP_TRY(tmp.alloc(&S, (size_t)n * np * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_s, (size_t)count * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_r, (size_t)count * sizeof(int64_t)));
  int rc = pairs_block_device(idx, c, variant, n, count, S, qbuf, d_s, d_r, st);
  if (rc != SVS_OK) return rc;
  std::vector<int64_t> flat_rows((size_t)count);
  HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(flat_rows.data(), d_r, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if ((rc = fr.wait()) != SVS_OK) return rc;
  for (int t = 0; t < count; ++t) {
    out_i[t] = flat_rows[t] / np + idx->row_offset;
    out_j[t] = flat_rows[t] % np + idx->row_offset;
  }
  return SVS_OK;
}

// Corpora whose n x n scores cannot be materialised (n^2 > 2^32: beyond ~65k rows; the reference
// itself stops at what fits its RAM).  (1) The exact count-th best pair score of a PREFIX block
// (rows [0, P), materialised as above) is a lower bound of the global count-th best.  (2) The
// tiled MFMA GEMM runs over chunks of query rows x the rows above them with the fused epilogue in
// pair mode: scores >= that bound and j > i become per-query candidates, nothing else is written;
// after each chunk they are appended to one global (score, i, j) list.  (3) The host orders the
// list by (score desc, i desc, j desc) -- the reference's flat upper-triangle index, descending --
// and keeps `count`.  Exact; the list holds about count * (n / P)^2 pairs.
int top_pairs_tiled(svs_index* idx, HostCall& fr, int variant, int count, float* out_scores, int64_t* out_i, int64_t* out_j) {
  const int64_t n = idx->n;
  constexpr int QC = 1024;                 // query rows per chunk
  // (every chunk holds more than GQ queries, so all take the family of a full one: it must have a pair mode)
  const BatchRoute::Family fam = batch_route(idx, variant, QC).family;
  if (fam != BatchRoute::TILED_F32 && fam != BatchRoute::TILED_EB) return fail(SVS_ERR_UNSUPPORTED, "pairwise scores over %lld rows need rows of whole 128-byte lines (d = %d)", (long long)n, idx->d);
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  int rc;
  // prefix block: at least `count` live pairs inside it
  int64_t P = std::min<int64_t>(n, count > SEL_KMAX ? 8192 : 16384);
  while (P < n && (P - (int64_t)idx->dead_list.size()) * (P - (int64_t)idx->dead_list.size() - 1) / 2 < count) P = std::min<int64_t>(n, P * 2);
  const int64_t Pp = score_stride(P);
  if (P * Pp > 0xffffffffll) return fail(SVS_ERR_UNSUPPORTED, "top_pairs: k = %d needs a prefix block past 2^32 scores", count);
  constexpr uint32_t LIST_CAP = 8u << 20;  // global pair list (96 MB)
  DevTmp tmp;
  float *qbuf = nullptr, *S = nullptr, *d_s = nullptr;
  int64_t* d_r = nullptr;
  uint32_t *gstate = nullptr, *l_key = nullptr, *l_i = nullptr, *l_j = nullptr;
  HIP_TRY(tmp.alloc(&qbuf, (size_t)QC * idx->d * sizeof(float)));
  HIP_TRY(tmp.alloc(&S, (size_t)P * Pp * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_s, (size_t)count * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_r, (size_t)count * sizeof(int64_t)));
  HIP_TRY(tmp.alloc(&gstate, 16));
  HIP_TRY(tmp.alloc(&l_key, (size_t)LIST_CAP * 4));
  HIP_TRY(tmp.alloc(&l_i, (size_t)LIST_CAP * 4));
  HIP_TRY(tmp.alloc(&l_j, (size_t)LIST_CAP * 4));
  HIP_TRY(hipMemsetAsync(gstate, 0, 16, st));
  if ((rc = pairs_block_device(idx, c, variant, P, count, S, qbuf, d_s, d_r, st)) != SVS_OK) return rc;
  const float* thr = d_s + (count - 1);    // the bound, read by the epilogue with stride 0
  // per-query candidate scratch for one chunk
  if ((rc = grow_select_scratch(c, QC, st)) != SVS_OK) return rc;
  for (int64_t q0 = 0; q0 < n - 1; q0 += QC) {
    // the last chunk is moved back so that it still holds QC rows (its first rows were done: first_query)
    const int64_t qs = std::max<int64_t>(0, std::min<int64_t>(q0, n - QC));
    const int nq = (int)std::min<int64_t>(QC, n - qs);
    const int64_t row_base = (qs + 1) & ~(int64_t)3;          // rows above the chunk's first query (4-aligned: fp8 row scales)
    if ((rc = dequant_rows_to(idx, qs, nq, qbuf, st)) != SVS_OK) return rc;
    FuseLaunch fl{c->hist, c->cand, thr, 0, TgPairs{(long long)qs, (long long)row_base, (long long)q0, 1}};
    if ((rc = score_batch(idx, c, variant, qbuf, nq, n - row_base, nullptr, 0, fl, st)) != SVS_OK) return rc;
    hipLaunchKernelGGL(collect_pairs_kernel, dim3(nq), dim3(256), 0, st, c->hist, (const uint64_t*)c->cand, (long long)qs, (long long)q0,
                       dead_bits_of(idx), gstate, LIST_CAP, l_key, l_i, l_j);
  }
  HIP_TRY(hipGetLastError());
  uint32_t hs[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(hs, gstate, 16, hipMemcpyDeviceToHost, st));
  if ((rc = fr.wait()) != SVS_OK) return rc;
  if (hs[1] || hs[0] > LIST_CAP)
    return fail(SVS_ERR_UNSUPPORTED, "top_pairs: more than %u pairs (or 32,768 for one row) score at least the %d-th best of the first %lld rows: "
                                      "near-duplicate documents en masse", LIST_CAP, count, (long long)P);
  const uint32_t L = hs[0];
  if ((int64_t)L < count) return fail(SVS_ERR_DEVICE, "internal: pair list holds %u < %d entries", L, count);
  std::vector<uint32_t> hk(L), hi(L), hj(L);
  HIP_TRY(hipMemcpy(hk.data(), l_key, (size_t)L * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hi.data(), l_i, (size_t)L * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hj.data(), l_j, (size_t)L * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> order(L);
  for (uint32_t t = 0; t < L; ++t) order[t] = t;
  auto before = [&](uint32_t a, uint32_t b) {   // (score desc, i desc, j desc)
    if (hk[a] != hk[b]) return hk[a] > hk[b];
    if (hi[a] != hi[b]) return hi[a] > hi[b];
    return hj[a] > hj[b];
  };
  std::partial_sort(order.begin(), order.begin() + count, order.end(), before);
  for (int t = 0; t < count; ++t) {
    out_scores[t] = key_score(hk[order[t]]);
    out_i[t] = (int64_t)hi[order[t]] + idx->row_offset;
    out_j[t] = (int64_t)hj[order[t]] + idx->row_offset;
  }
  return SVS_OK;
}

int check_query_args(const svs_index* idx, const void* q, int nq, int d) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (nq < 0) return fail(SVS_ERR_INVALID, "nq must be >= 0");
  if (d != idx->d || idx->n == 0 || idx->d == 0)
    return fail(SVS_ERR_SHAPE, "shapes (%lld,%d) and (%d,) not aligned: %d (dim 1) != %d (dim 0)",
                (long long)idx->n, idx->d, d, idx->d, d);
  if (nq > 0 && !q) return fail(SVS_ERR_INVALID, "null queries");
  return SVS_OK;
}

// f32 source rows [0, nrows) with a stride of src_ld floats -> rows [row0, row0 + nrows) of the corpus layout, on `st`.
// f32 corpus: a copy of `kind` (the source is device or pinned memory) that writes the d floats of every row; the
// columns of padded rows beyond d are the caller's to zero.  f16 / fp8 corpus: the source is on the device and a kernel
// of `blocks` workgroups converts it.
// ... into rows [row0, row0 + nrows) of ANY image of the index's layout: `rows` (stride idx->ld elements) and, fp8, `scales`
// (the corpus itself; svs_index_assign's image of its vectors)
hipError_t ingest_rows_into(const svs_index* idx, void* rows, float* scales, const float* src, int64_t nrows, int64_t src_ld, int64_t row0,
                            hipMemcpyKind kind, unsigned blocks, hipStream_t st) {
  const int d = idx->d;
  if (idx->dtype == SVS_DTYPE_F16) {
    hipLaunchKernelGGL(convert_rows_f16_kernel, dim3(blocks), dim3(256), 0, st, src, nrows, d, src_ld,
                       (_Float16*)rows + (size_t)row0 * idx->ld, idx->ld);
    return hipGetLastError();
  }
  if (idx->dtype == SVS_DTYPE_FP8) {
    hipLaunchKernelGGL(quantize_rows_fp8_kernel, dim3(blocks), dim3(256), 0, st, src, nrows, d, src_ld,
                       (uint8_t*)rows + (size_t)row0 * idx->ld, idx->ld, scales + row0, (float*)nullptr);
    return hipGetLastError();
  }
  float* dst = (float*)rows + (size_t)row0 * idx->ld;
  if (kind == hipMemcpyHostToDevice && idx->ld == d && src_ld == d)
    return hipMemcpyAsync(dst, src, (size_t)nrows * d * sizeof(float), kind, st);
  return hipMemcpy2DAsync(dst, (size_t)idx->ld * sizeof(float), src, (size_t)src_ld * sizeof(float), (size_t)d * sizeof(float),
                          (size_t)nrows, kind, st);
}
hipError_t ingest_rows(svs_index* idx, const float* src, int64_t nrows, int64_t src_ld, int64_t row0, hipMemcpyKind kind,
                       unsigned blocks, hipStream_t st) {
  return ingest_rows_into(idx, idx->rows, idx->row_scales, src, nrows, src_ld, row0, kind, blocks, st);
}

// Host rows [0, nrows) (f32, C-contiguous, d floats each) -> HBM rows [row0, row0+nrows).
// Pinned double-buffered staging: host memcpy of chunk i+1 overlaps the DMA of chunk i.
// f32 corpus: the DMA writes the padded HBM layout directly (2D copy).
// f16 / fp8 corpus: the DMA lands in a device staging buffer and a kernel converts it.
hipError_t upload_host_rows(svs_index* idx, const float* host_rows, int64_t nrows, int64_t row0) {
  const int d = idx->d;
  const int64_t n = nrows;
  const bool f16 = idx->dtype != SVS_DTYPE_F32;   // f16 and fp8: convert on the device
  const size_t row_b = (size_t)d * sizeof(float);
  const size_t esz = elem_bytes(idx);
  const size_t chunk_rows = std::max<size_t>(1, std::min<size_t>((32u << 20) / row_b, (size_t)n));
  void* pin[2] = {nullptr, nullptr};
  float* dstage[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  hipStream_t st = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipHostMalloc(&pin[i], chunk_rows * row_b, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
    if (e == hipSuccess && f16) e = hipMalloc((void**)&dstage[i], chunk_rows * row_b);
  }
  if (e == hipSuccess && !f16 && idx->ld != d)
    e = hipMemsetAsync((char*)idx->rows + (size_t)row0 * idx->ld * esz, 0, (size_t)n * idx->ld * esz, st);
  int b = 0;
  for (size_t r0 = 0; r0 < (size_t)n && e == hipSuccess; r0 += chunk_rows, b ^= 1) {
    const size_t rows = std::min(chunk_rows, (size_t)n - r0);
    const size_t dr = (size_t)row0 + r0;   // destination row
    e = hipEventSynchronize(done[b]);
    if (e != hipSuccess) break;
    memcpy(pin[b], host_rows + r0 * (size_t)d, rows * row_b);
    if (f16) e = hipMemcpyAsync(dstage[b], pin[b], rows * row_b, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ingest_rows(idx, f16 ? dstage[b] : (const float*)pin[b], (int64_t)rows, d, (int64_t)dr, hipMemcpyHostToDevice, 2048, st);
    if (e == hipSuccess) e = hipEventRecord(done[b], st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (int i = 0; i < 2; ++i) {
    if (done[i]) (void)hipEventDestroy(done[i]);
    if (pin[i]) (void)hipHostFree(pin[i]);
    if (dstage[i]) (void)hipFree(dstage[i]);
  }
  if (st) (void)hipStreamDestroy(st);
  return e;
}


// Row stride in elements.  Rows are always 16-byte aligned (4 floats / 8 halves / 16 fp8).
//  1. A whole number of 1 KiB wave loads when that costs at most an eighth more bytes (zero
//     columns): the exact-geometry streaming kernels, ~7 TB/s (d = 1000 -> 1024: +2.4 %).
//  2. Otherwise whole 128-byte lines per row, again for at most an eighth more: rows then never
//     share a cache line (the streams are nontemporal), the tiled kernels' 128-byte k-steps
//     apply, and gemv_unrolled.h streams such rows at 6.6-7.1 TB/s (d = 384 f16: 768-byte rows;
//     the earlier rule padded them to 1 KiB, +33 % bytes).
//  3. Otherwise tight.
int choose_ld(int d, int dtype) {
  const int align = 16 / (int)dtype_bytes(dtype);   // elements per 16 bytes
  const int tight = (d + align - 1) / align * align;
  if (d <= 0) return tight;
  const int wave = 64 * align, line = 8 * align;
  const int waved = (d + wave - 1) / wave * wave, lined = (d + line - 1) / line * line;
  if ((int64_t)waved * 8 <= (int64_t)tight * 9) return waved;
  if ((int64_t)lined * 8 <= (int64_t)tight * 9) return lined;
  return tight;
}

// ---- the half shadow of an f32 corpus (screen.h): ingest side ----------------------------------
bool shadow_eligible(const svs_index* idx) {
  return idx->dtype == SVS_DTYPE_F32 && idx->d > 0 && idx->ld % 512 == 0 && idx->ld <= 4096 &&
         choose_ld(idx->d, SVS_DTYPE_F16) == idx->ld;   // a hot geometry of the f16 one-shot kernel, same stride as the f32 rows
}

void shadow_free(svs_index* idx) {
  idx->geo_epoch.fetch_add(1);
  (void)hipFree(idx->shadow);
  idx->shadow = nullptr;
  idx->shadow_bytes = 0;
}

// Best effort: false (and no shadow) when HBM is short.  Never leaves a HIP error behind.
bool shadow_alloc(svs_index* idx, int64_t rows_cap, void** out) {
  *out = nullptr;
  if (g_tune_refuse_shadow.load() || rows_cap <= 0) return false;
  if (!idx->scr_dev) {
    const size_t words = sizeof(ScreenStats) / 4 + (size_t)svs_index::kSlots * SCREEN_SLOT_WORDS;
    if (hipMalloc((void**)&idx->scr_dev, words * 4) != hipSuccess || hipMemset(idx->scr_dev, 0, words * 4) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(idx->scr_dev);
      idx->scr_dev = nullptr;
      return false;
    }
  }
  if (!idx->scr_host) {
    const size_t bytes = (size_t)svs_index::kSlots * SCREEN_SLOT_WORDS * 4;
    if (hipHostMalloc((void**)&idx->scr_host, bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      idx->scr_host = nullptr;
      return false;
    }
    memset(idx->scr_host, 0, bytes);
  }
  if (hipMalloc(out, (size_t)rows_cap * idx->ld * sizeof(_Float16)) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return false;
  }
  return true;
}

// Rows [row0, row0 + nrows) of idx->rows were written (or are being written, in order, on `st`): convert them into
// the shadow on `st`.  A handle that has no shadow yet (created empty, or after set_screen(1)) gets one over all
// n_total rows.  sync: wait for the conversion and read the `bad` flag back (every ingest path but the staging commit,
// whose flag is read when the staging stream is next drained).  Caller holds the geometry lock exclusively.
void shadow_ingest(svs_index* idx, int64_t row0, int64_t nrows, int64_t n_total, hipStream_t st, bool sync) {
  idx->scr_paused.store(false);   // new rows: whatever made the fallbacks dominate may be gone
  idx->geo_epoch.fetch_add(1);    // (every ingest path comes by here: n, the rows or the shadow change)
  if (!shadow_eligible(idx) || idx->screen_mode.load() != 1 || idx->shadow_bad.load() || idx->shadow_gave_up) return;
  if (!idx->shadow) {
    void* sh = nullptr;
    if (!shadow_alloc(idx, std::max(idx->cap, n_total), &sh)) {
      idx->shadow_gave_up = true;
      return;
    }
    idx->shadow = sh;
    idx->shadow_bytes = (size_t)std::max(idx->cap, n_total) * idx->ld * sizeof(_Float16);
    if (hipMemsetAsync(idx->scr_dev, 0, sizeof(ScreenStats), st) != hipSuccess) (void)hipGetLastError();
    row0 = 0;
    nrows = n_total;
  }
  if (nrows <= 0) return;
  const int blocks = (int)std::min<int64_t>((nrows + 3) / 4, (int64_t)idx->cu_count * 8);
  hipLaunchKernelGGL(shadow_rows_kernel, dim3(blocks), dim3(256), 0, st, (const v4f*)idx->rows, row0, nrows, idx->ld / 4,
                     (uint2*)idx->shadow, (ScreenStats*)idx->scr_dev);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && sync) {
    ScreenStats h{};
    e = hipMemcpyAsync(&h, idx->scr_dev, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && h.bad) idx->shadow_bad.store(true);
  } else if (e == hipSuccess) {
    idx->stats_dirty = true;
  }
  if (e != hipSuccess) {   // never a new failure: search unscreened
    (void)hipGetLastError();
    idx->shadow_bad.store(true);
  }
  if (idx->shadow_bad.load() && sync) shadow_free(idx);   // (nothing reads a shadow that never screens)
}

// Device rows [0, nrows) (f32, stride src_ld) -> HBM rows [row0, row0 + nrows) of the index's layout.
hipError_t copy_device_rows(svs_index* idx, const float* dev_rows, int64_t nrows, int64_t src_ld, int64_t row0) {
  hipError_t e = hipSuccess;
  if (idx->dtype == SVS_DTYPE_F32 && idx->ld != idx->d)
    e = hipMemset((float*)idx->rows + (size_t)row0 * idx->ld, 0, (size_t)nrows * idx->ld * sizeof(float));
  if (e == hipSuccess) e = ingest_rows(idx, dev_rows, nrows, src_ld, row0, hipMemcpyDeviceToDevice, 4096, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}

// Room for `need` words in a device buffer that enqueued searches may still read: drained before it is replaced
// (caller holds the geometry lock exclusively).
int grow_drained(DevBuf<uint32_t>& buf, size_t need) {
  if (need <= buf.cap) return SVS_OK;
  HIP_TRY(hipDeviceSynchronize());
  return buf.grow(need);
}

// Device bitmap of the masked rows, one bit per row of the current capacity (caller holds the
// geometry lock exclusively).  Nothing is allocated while no row is masked.
int sync_dead_bits(svs_index* idx) {
  if (idx->dead_list.empty()) return SVS_OK;
  const size_t words = (size_t)((std::max(idx->cap, idx->n) + 31) / 32);
  idx->dead_bits.assign(words, 0u);
  for (uint32_t r : idx->dead_list) idx->dead_bits[r >> 5] |= 1u << (r & 31);
  int rc = grow_drained(idx->dead_bits_dev, words);
  if (rc != SVS_OK) return rc;
  HIP_TRY(hipMemcpy(idx->dead_bits_dev, idx->dead_bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  return SVS_OK;
}

// ---- the label column and its ordered filter (labels.h) ------------------------------------------------------------
static_assert(SVS_LABELS_MAX_SET == LB_MAX_SET, "the filter kernels' LDS image of the set holds SVS_LABELS_MAX_SET labels");
constexpr size_t label_column_bytes(int64_t rows_cap) { return (size_t)((rows_cap + 3) & ~(int64_t)3) * sizeof(uint32_t); }
inline int64_t label_strips(int64_t n) { return (n + LB_STRIP - 1) / LB_STRIP; }

// The filter over the rows [0, n) the index holds: set[0 .. nset) sorted and distinct on the HOST, set_dev its device
// copy (read when nset >= 2 only); nset == 0: every live row
LabelFilter label_filter(const svs_index* idx, int column, const uint32_t* set, int nset, const uint32_t* set_dev) {
  return LabelFilter{idx->cols[column], idx->n, dead_bits_of(idx), set_dev, nset, nset == 1 ? set[0] : 0u};
}

// The two kernels of a filter type (labels.h's strip compaction; where.h's writes rows only)
inline auto strip_count_kernel(const LabelFilter&) { return &label_count_kernel; }
inline auto strip_count_kernel(const WhereFilter&) { return &where_count_kernel; }
template <int PAYLOAD> auto strip_write_kernel(const LabelFilter&) { return &label_write_kernel<PAYLOAD>; }
template <int PAYLOAD> auto strip_write_kernel(const WhereFilter&) {
  static_assert(PAYLOAD == LB_ROWS, "where_write_kernel writes row indices");
  return &where_write_kernel;
}

// cnt: one u64 (the total, zeroed here) followed by one u32 per strip of f.n rows
template <class FILTER>
void launch_label_count(const FILTER& f, uint32_t* cnt, hipStream_t st) {
  (void)hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st);
  hipLaunchKernelGGL(strip_count_kernel(f), dim3((unsigned)label_strips(f.n)), dim3(LB_THREADS), 0, st, f, cnt + 2, (unsigned long long*)cnt);
}

// ... and behind it: the counts scanned into the strips' bases, then the m matches written to out in ascending row order
template <int PAYLOAD, class FILTER>
void launch_label_write(const FILTER& f, uint32_t* cnt, uint32_t* out, int64_t m, hipStream_t st) {
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(LB_THREADS), 0, st, cnt + 2, label_strips(f.n));
  hipLaunchKernelGGL(strip_write_kernel<PAYLOAD>(f), dim3((unsigned)label_strips(f.n)), dim3(LB_THREADS), 0, st, f, (const uint32_t*)(cnt + 2), out, m);
}

// A caller's label set, sorted and without repeats: a label's SLOT in every table of the device is its index here
struct LabelSet {
  using Filter = LabelFilter;
  std::vector<uint32_t> set;
  int nset = 0;
  // The caller's arguments, checked where the entry checked them; build (entry: the ABI name, for the message) follows
  static int check(const uint32_t* labels, int32_t nlabels) {
    if (nlabels < 0) return fail(SVS_ERR_INVALID, "nlabels must be >= 0");
    return nlabels > 0 && !labels ? fail(SVS_ERR_INVALID, "null labels") : (int)SVS_OK;
  }
  // set = the distinct members of labels[0 .. nlabels), ascending (std::bad_alloc is the caller's to report)
  static void sort_distinct(std::vector<uint32_t>& set, const uint32_t* labels, int32_t nlabels) {
    set.assign(labels, labels + nlabels);
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
  }
  int build(const char* entry, const uint32_t* labels, int32_t nlabels) {
    try {
      sort_distinct(set, labels, nlabels);
    } catch (const std::bad_alloc&) {
      return fail(SVS_ERR_NOMEM, "out of host memory for %d labels", (int)nlabels);
    }
    if (set.size() > (size_t)SVS_LABELS_MAX_SET)
      return fail(SVS_ERR_UNSUPPORTED, "%s: %zu distinct labels; a set holds at most %d", entry, set.size(), SVS_LABELS_MAX_SET);
    nset = (int)set.size();
    return SVS_OK;
  }
  size_t slot_of(uint32_t label) const { return (size_t)(std::lower_bound(set.begin(), set.end(), label) - set.begin()); }
  // Two labels or more go up on st through the context's pinned copy (one is a kernel argument); *f = the index's filter
  int stage(const svs_index* idx, Ctx* c, hipStream_t st, LabelFilter* f) const {
    if (nset >= 2) {
      int rc;
      if ((rc = c->lab_set_pin.grow((size_t)nset)) != SVS_OK || (rc = c->lab_set_dev.grow((size_t)nset)) != SVS_OK) return rc;
      memcpy(c->lab_set_pin, set.data(), (size_t)nset * sizeof(uint32_t));
      HIP_TRY(hipMemcpyAsync(c->lab_set_dev, c->lab_set_pin, (size_t)nset * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    *f = label_filter(idx, 0, set.data(), nset, c->lab_set_dev);
    return SVS_OK;
  }
};

// The local range of a caller's [row0, row0 + nrows) of GLOBAL rows: nrows < 0 is refused, and so is a range, empty or
// not, that is not inside the index
int label_range(const svs_index* idx, const char* entry, int64_t row0, int64_t nrows, int64_t* r0) {
  if (nrows < 0) return fail(SVS_ERR_INVALID, "nrows must be >= 0");
  *r0 = row0 - idx->row_offset;
  if (*r0 < 0 || *r0 > idx->n || nrows > idx->n - *r0)
    return fail(SVS_ERR_INVALID, "%s: rows [%lld, %lld) outside [%lld, %lld)", entry, (long long)row0, (long long)(row0 + nrows),
                (long long)idx->row_offset, (long long)(idx->row_offset + idx->n));
  return SVS_OK;
}

// The entries that gather rows (gather.h) refuse rows no gather kernel takes
int check_gather_rows(const svs_index* idx, const char* entry) {
  return gather_rows_per_wave(idx) != 0 ? (int)SVS_OK
      : fail(SVS_ERR_UNSUPPORTED, "%s: rows of %zu bytes; the gather kernels take rows of up to 16 KiB", entry, (size_t)idx->ld * elem_bytes(idx));
}

// Per-query cut-offs (svs_index_search_above, svs_index_search_by_label): none may be NaN; null: no cut-offs
int check_cutoffs(const char* entry, const float* min_scores, int32_t nq) {
  for (int32_t q = 0; min_scores && q < nq; ++q)
    if (min_scores[q] != min_scores[q]) return fail(SVS_ERR_INVALID, "%s: the cut-off of query %d is NaN", entry, (int)q);
  return SVS_OK;
}

// Uploaded query q (c->q_dev) scored into the context's one score vector
int launch_query_scores(const svs_index* idx, Ctx* c, const SingleRoute& route, int32_t q, hipStream_t st) {
  launch_record("gemv", idx->n, 1);
  return launch_scores(idx, c, route, c->q_dev + (size_t)q * idx->d, c->scores, st);
}

// ---- svs_index_search_combined (combine.h) -------------------------------------------------------------------------
static_assert(SVS_COMBINE_MAX == CB_MAX && SVS_COMBINE_MIN == CB_MIN && SVS_COMBINE_SUM == CB_SUM && SVS_COMBINE_MAX_VECTORS == CB_MAX_VECTORS,
              "combine.h's kernels take the header's op codes and limit");
static_assert(CB_MAX_VECTORS <= GQ, "the padded vectors of a combined query are staged in Ctx::q16");

// The route of a combined query, decided once per call: the fused kernel of the index's one-shot family, or m passes of
// `single` -- the kernel svs_index_scores_n runs -- and combine_scores_kernel.
struct CombineRoute {
  bool fused;           // what the call runs
  bool has_fused;       // the row length has a fused kernel
  SingleRoute single;
};
// The fused kernels' names, as c++filt prints them: the geometry is the single-query one-shot kernels' (f32: launch_rows' default)
template <int NSTEP>
constexpr KernelName kCombineF32Name = kernel_name("combine_f32_kernel", NSTEP, f32_rows_r(NSTEP), f32_rows_wpb(NSTEP));
template <int NSTEP>
constexpr KernelName kCombineF16Name = kernel_name("combine_f16_kernel", NSTEP, f16_rows_r(NSTEP), f16_rows_wpb(NSTEP));
template <int NSTEP, int LB, int R>
constexpr KernelName kCombineFp8Name = kernel_name("combine_fp8_kernel", NSTEP, LB, R, 16);
template <int NSTEP>
constexpr KernelName kMultiScoreF32Name = kernel_name("multi_score_f32_kernel", NSTEP, f32_rows_r(NSTEP), f32_rows_wpb(NSTEP));
template <int NSTEP>
constexpr KernelName kMultiScoreF16Name = kernel_name("multi_score_f16_kernel", NSTEP, f16_rows_r(NSTEP), f16_rows_wpb(NSTEP));
template <int NSTEP, int LB, int R>
constexpr KernelName kMultiScoreFp8Name = kernel_name("multi_score_fp8_kernel", NSTEP, LB, R, 16);

// Where the fused route is the default, per dtype and m: where it was measured FASTER than the passes (1M x 1536,
// profiles/combined_time.txt) -- from two vectors on, in all three dtypes.  One vector: a tie within the
// spread for f32 and f16, and the passes ahead for fp8; it takes the passes.
inline bool combine_fused_default(int /*dtype*/, int m) { return m >= 2; }

// force: 0 the route's choice, 1 fused where a fused kernel exists, 2 passes
CombineRoute combine_route(const svs_index* idx, int variant, int m, int force) {
  const SingleRoute s = single_route(idx, variant, false);
  // (a geometry A/B variant of the single-query kernels, 1 .. 5, keeps to the passes: its kernels are what is being compared)
  const bool geometry_ab = variant >= VARIANT_GEMV_PERSISTENT_R1 && variant <= VARIANT_GEMV_1X8;
  const bool has = (s.family == SingleRoute::F32_ROWS && s.geo >= 1 && s.geo <= 16) || (s.family == SingleRoute::F16_ONESHOT && s.geo >= 1 && s.geo <= 8) ||
                   s.family == SingleRoute::FP8_ONESHOT;
  const bool fused = has && force != 2 && (force == 1 || (!geometry_ab && combine_fused_default(idx->dtype, m)));
  return CombineRoute{fused, has, s};
}

// Where the scores of a combined query's m vectors go
struct ScoreSink {
  bool fold;        // folded under (w, op) into c->scores[0 .. n); else vector j's stored apart, at c->scores[j * sstride ..)
  const float* w;   // fold: the query's m weights on the device
  int op;
};
constexpr ScoreSink kStoreScores{false, nullptr, 0};

// The m vectors of one combined query scored on route r, unmasked, into the sink.  v: the vectors on the device, [m][d].
// c->scores holds m * sstride floats (a fused fold needs one vector's; the passes' fold ends up in the first of the m).
// One staging and one geometry per dtype; the sink picks between the two families of fused kernels (combine.h).
int enqueue_vector_scores(const svs_index* idx, Ctx* c, const CombineRoute& r, const float* v, int m, int64_t sstride, const ScoreSink& sink,
                          hipStream_t st) {
  const int64_t n = idx->n;
  int rc;
  if (!r.fused) {
    for (int j = 0; j < m; ++j) {
      launch_record("gemv", n, 1);
      if ((rc = launch_scores(idx, c, r.single, v + (size_t)j * idx->d, c->scores + (size_t)j * sstride, st)) != SVS_OK) return rc;
    }
    if (!sink.fold) return SVS_OK;
    launch_record("combine_scores_kernel", n, m);
    const int64_t n4 = sstride >> 2;
    hipLaunchKernelGGL(combine_scores_kernel, dim3((unsigned)std::min<int64_t>((n4 + 255) / 256, 4096)), dim3(256), 0, st, c->scores.p, sstride, n4, m, sink.w,
                       sink.op);
    return SVS_OK;
  }
  // The sink's kernel of a family over the one-shot grid: the rows and the staged vectors, then what the sink adds
  const auto launch = [&](const KernelName& fold_name, auto fold_kernel, const KernelName& store_name, auto store_kernel, int rows_per_block, int threads,
                          auto... rows_and_vectors) {
    const dim3 grid((unsigned)((n + rows_per_block - 1) / rows_per_block));
    launch_record(sink.fold ? fold_name.s : store_name.s, n, m);
    if (sink.fold) hipLaunchKernelGGL(fold_kernel, grid, dim3(threads), 0, st, rows_and_vectors..., sink.w, m, sink.op, c->scores.p, n);
    else hipLaunchKernelGGL(store_kernel, grid, dim3(threads), 0, st, rows_and_vectors..., m, c->scores.p, sstride, n);
  };
  bool ok;
  if (r.single.family == SingleRoute::FP8_ONESHOT) {
    if ((rc = stage_queries_fp8(idx, c, v, m, m, false, st)) != SVS_OK) return rc;
    ok = for_fp8_oneshot(idx->ld, [&](auto ns, auto lb, auto rr) {
      constexpr int NSTEP = ns(), LB = lb(), R = rr();
      launch(kCombineFp8Name<NSTEP, LB, R>, combine_fp8_kernel<NSTEP, LB, R, 16>, kMultiScoreFp8Name<NSTEP, LB, R>, multi_score_fp8_kernel<NSTEP, LB, R, 16>,
             R * 16, 16 * 64, (const uint8_t*)idx->rows, (const float*)idx->row_scales, (const uint8_t*)c->q8.p, (const float*)c->q8s.p);
    });
  } else {
    // f32 / f16: the vectors as ld floats each, 16-byte aligned -- the caller's where the rows are not padded
    const float* q = v;
    if (query_needs_copy(idx, v)) {
      if ((rc = c->q16.grow((size_t)GQ * idx->ld)) != SVS_OK) return rc;
      HIP_TRY(hipMemsetAsync(c->q16, 0, (size_t)m * idx->ld * sizeof(float), st));
      HIP_TRY(hipMemcpy2DAsync(c->q16, (size_t)idx->ld * sizeof(float), v, (size_t)idx->d * sizeof(float), (size_t)idx->d * sizeof(float), (size_t)m,
                               hipMemcpyDeviceToDevice, st));
      q = c->q16;
    }
    if (r.single.family == SingleRoute::F16_ONESHOT)
      ok = for_f16_oneshot(r.single.geo, [&](auto ns) {
        constexpr int NSTEP = ns(), R = f16_rows_r(NSTEP), WPB = f16_rows_wpb(NSTEP);
        launch(kCombineF16Name<NSTEP>, combine_f16_kernel<NSTEP, R, WPB>, kMultiScoreF16Name<NSTEP>, multi_score_f16_kernel<NSTEP, R, WPB>, R * WPB, WPB * 64,
               (const u32x4*)idx->rows, (const v4f*)q);
      });
    else
      ok = for_f32_rows(r.single.geo, [&](auto ns) {
        constexpr int NSTEP = ns(), R = f32_rows_r(NSTEP), WPB = f32_rows_wpb(NSTEP);
        launch(kCombineF32Name<NSTEP>, combine_f32_kernel<NSTEP, R, WPB>, kMultiScoreF32Name<NSTEP>, multi_score_f32_kernel<NSTEP, R, WPB>, R * WPB, WPB * 64,
               (const v4f*)idx->rows, (const v4f*)q);
      });
  }
  return ok ? SVS_OK : fail(SVS_ERR_INVALID, "internal: no fused kernel for ld %d", idx->ld);
}

// The arguments every combined entry takes, checked in the header's order; `entry` names the caller
int check_combined_args(const char* entry, const svs_index* idx, const float* vectors, int64_t nq, int32_t m, int32_t d, const float* weights, int32_t op) {
  if (nq < 0) return fail(SVS_ERR_INVALID, "%s: nq must be >= 0", entry);
  if (m < 1 || m > SVS_COMBINE_MAX_VECTORS) return fail(SVS_ERR_INVALID, "%s: m is %d, a combined query has 1 .. %d vectors", entry, (int)m, SVS_COMBINE_MAX_VECTORS);
  if (d != idx->d) return fail(SVS_ERR_INVALID, "%s: d is %d, the index holds rows of %d", entry, (int)d, idx->d);
  if (op != SVS_COMBINE_MAX && op != SVS_COMBINE_MIN && op != SVS_COMBINE_SUM) return fail(SVS_ERR_INVALID, "%s: unknown op %d", entry, (int)op);
  if (nq > 0 && !vectors) return fail(SVS_ERR_INVALID, "%s: null vectors", entry);
  for (int64_t i = 0; weights && i < nq * m; ++i)
    if (!std::isfinite(weights[i]))
      return fail(SVS_ERR_INVALID, "%s: weights: the weight of vector %d of query %lld is not finite", entry, (int)(i % m), (long long)(i / m));
  return SVS_OK;
}

// The call's vectors and weights (null: 1.0f each) to the device in one copy: c->q_dev = [nq * m * d vectors | nq * m weights]
int upload_combined(Ctx* c, const float* vectors, const float* weights, size_t vn, size_t wn, hipStream_t st) {
  int rc;
  if ((rc = c->q_dev.grow(vn + wn)) != SVS_OK || (rc = c->q_pin.grow(vn + wn)) != SVS_OK) return rc;
  memcpy(c->q_pin, vectors, vn * sizeof(float));
  if (weights) memcpy(c->q_pin + vn, weights, wn * sizeof(float));
  else std::fill(c->q_pin + vn, c->q_pin + vn + wn, 1.0f);
  HIP_TRY(hipMemcpyAsync(c->q_dev, c->q_pin, (vn + wn) * sizeof(float), hipMemcpyHostToDevice, st));
  return SVS_OK;
}

// svs_index_set_timing: the two events around a call's kernels, made only when wanted (the index is timed and the call
// runs what is timed) and destroyed on every exit.  ms(), once the stream has drained: begin to end, or -1.
struct TimedSpan {
  hipEvent_t ev[2] = {nullptr, nullptr};
  const bool on;
  explicit TimedSpan(bool wanted) : on(wanted && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess) {}
  ~TimedSpan() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  void begin(hipStream_t st) const { if (on) (void)hipEventRecord(ev[0], st); }
  void end(hipStream_t st) const { if (on) (void)hipEventRecord(ev[1], st); }
  double ms() const { float t = 0.f; return on && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess ? (double)t : -1.0; }
};

// Behind a call's launches: they were accepted, the copies are enqueued (a null dst: nobody asked), the stream drains
struct ReadBack { void* dst; const void* src; size_t bytes; };
int read_back(HostCall& fr, const char* entry, std::initializer_list<ReadBack> copies) {
  int rc = fr.launched(entry);
  for (const ReadBack& r : copies) {
    const hipError_t e = rc == SVS_OK && r.dst ? hipMemcpyAsync(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost, fr.stream()) : hipSuccess;
    if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? SVS_ERR_NOMEM : SVS_ERR_DEVICE, "%s read-back: %s", entry, hipGetErrorString(e));
  }
  return rc == SVS_OK ? fr.wait() : rc;
}

// Makes room for `rows` rows (caller holds the geometry lock exclusively).  exact == false grows
// by 1.5x (amortised appends); exact == true (svs_index_reserve) allocates just `rows`.
int ensure_capacity(svs_index* idx, int64_t rows, bool exact) {
  if (rows > 0xffffffffll) return fail(SVS_ERR_INVALID, "at most 2^32 rows per handle; shard the corpus");
  if (rows <= idx->cap) return SVS_OK;
  const size_t row_b = (size_t)idx->ld * elem_bytes(idx);
  const int64_t new_cap = exact ? rows : std::max<int64_t>(rows, idx->cap + idx->cap / 2 + 1024);
  void* nrows = nullptr;
  float* nscales = nullptr;
  HIP_TRY(hipMalloc(&nrows, (size_t)new_cap * row_b));
  if (idx->dtype == SVS_DTYPE_FP8) {
    hipError_t e = hipMalloc((void**)&nscales, (size_t)new_cap * sizeof(float));
    if (e != hipSuccess) {
      (void)hipFree(nrows);
      return fail(SVS_ERR_NOMEM, "hipMalloc(row scales): %s", hipGetErrorString(e));
    }
  }
  // (the new buffers are the caller's problem only once they are installed: every failure until then frees them)
  struct Fresh {
    void* rows; float* scales; uint32_t* cols[SVS_COLUMNS_MAX] = {}; bool keep = false;
    ~Fresh() { if (!keep) { (void)hipFree(rows); (void)hipFree(scales); for (uint32_t* col : cols) (void)hipFree(col); } }
  } fresh{nrows, nscales};
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {   // every column the index owns grows with the rows: the old values, then zeros
    if (!idx->cols[c]) continue;
    const hipError_t e = hipMalloc((void**)&fresh.cols[c], label_column_bytes(new_cap));
    if (e != hipSuccess) return fail(SVS_ERR_NOMEM, "hipMalloc(column %d): %s", c, hipGetErrorString(e));
  }
  // work already enqueued by the device API may still read the old buffers
  HIP_TRY(hipDeviceSynchronize());
  const int64_t n_old = idx->n;
  if (n_old) HIP_TRY(hipMemcpy(nrows, idx->rows, (size_t)n_old * row_b, hipMemcpyDeviceToDevice));
  if (n_old && nscales) HIP_TRY(hipMemcpy(nscales, idx->row_scales, (size_t)n_old * sizeof(float), hipMemcpyDeviceToDevice));
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {
    if (!fresh.cols[c]) continue;
    HIP_TRY(hipMemset(fresh.cols[c], 0, label_column_bytes(new_cap)));
    if (n_old) HIP_TRY(hipMemcpy(fresh.cols[c], idx->cols[c], (size_t)n_old * sizeof(uint32_t), hipMemcpyDeviceToDevice));
  }
  fresh.keep = true;
  (void)hipFree(idx->rows);
  (void)hipFree(idx->row_scales);
  idx->rows = nrows;
  idx->row_scales = nscales;
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {
    (void)hipFree(idx->cols[c]);
    idx->cols[c] = fresh.cols[c];
    idx->col_bytes[c] = fresh.cols[c] ? label_column_bytes(new_cap) : 0;
  }
  if (idx->shadow) {   // grows with the rows; if there is no room for it the index carries on without
    void* nsh = nullptr;
    bool ok = shadow_alloc(idx, new_cap, &nsh);
    if (ok && n_old && hipMemcpy(nsh, idx->shadow, (size_t)n_old * idx->ld * sizeof(_Float16), hipMemcpyDeviceToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(nsh);
      ok = false;
    }
    shadow_free(idx);
    if (ok) {
      idx->shadow = nsh;
      idx->shadow_bytes = (size_t)new_cap * idx->ld * sizeof(_Float16);
    } else {
      idx->shadow_gave_up = true;
    }
  }
  idx->cap = new_cap;
  idx->bytes = (size_t)new_cap * row_b + (idx->dtype == SVS_DTYPE_FP8 ? (size_t)new_cap * sizeof(float) : 0);
  return SVS_OK;
}

int create_common(int64_t n, int32_t d, int32_t store_dtype, int32_t device, int64_t row_offset,
                  svs_index** out, svs_index** made) {
  if (!out) return fail(SVS_ERR_INVALID, "null out");
  *out = nullptr;
  if (n < 0 || d < 0) return fail(SVS_ERR_INVALID, "negative shape (%lld, %d)", (long long)n, d);
  if (store_dtype != SVS_DTYPE_F32 && store_dtype != SVS_DTYPE_F16 && store_dtype != SVS_DTYPE_FP8)
    return fail(SVS_ERR_UNSUPPORTED, "unknown store dtype %d", store_dtype);
  if (n > 0xffffffffll) return fail(SVS_ERR_INVALID, "at most 2^32 rows per handle; shard the corpus");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SVS_ERR_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(SVS_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  svs_index* idx = new (std::nothrow) svs_index();
  if (!idx) return fail(SVS_ERR_NOMEM, "host allocation failed");
  idx->device = device;
  idx->n = n;
  idx->cap = n;
  idx->d = d;
  idx->dtype = store_dtype;
  idx->ld = choose_ld(d, store_dtype);
  idx->row_offset = row_offset;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) idx->cu_count = prop.multiProcessorCount;
  idx->bytes = (size_t)n * (size_t)idx->ld * elem_bytes(idx);
  if (idx->bytes) {
    hipError_t e = hipMalloc(&idx->rows, idx->bytes);
    if (e != hipSuccess) {
      delete idx;
      return fail(e == hipErrorOutOfMemory ? SVS_ERR_NOMEM : SVS_ERR_DEVICE, "hipMalloc(%zu): %s", idx->bytes, hipGetErrorString(e));
    }
    if (store_dtype == SVS_DTYPE_FP8) {
      e = hipMalloc((void**)&idx->row_scales, (size_t)n * sizeof(float));
      if (e != hipSuccess) {
        (void)hipFree(idx->rows);
        delete idx;
        return fail(SVS_ERR_NOMEM, "hipMalloc(row scales): %s", hipGetErrorString(e));
      }
      idx->bytes += (size_t)n * sizeof(float);
    }
  }
  idx->dead_flag.assign((size_t)n, 0);
  if (const char* env = getenv("SVS_AMD_SCREEN")) idx->screen_mode.store(atoi(env) != 0 ? 1 : 0);
  *made = idx;
  return SVS_OK;
}

// svs_index_create / _from_device: fill(idx) checks the source and brings rows [0, n) in (SVS_OK, or the failure as
// it has reported it)
template <class Fill>
int create_index(int64_t n, int32_t d, int32_t store_dtype, int32_t device, int64_t row_offset, svs_index** out, Fill fill) {
  svs_index* idx = nullptr;
  int rc = create_common(n, d, store_dtype, device, row_offset, out, &idx);
  if (rc != SVS_OK) return rc;
  if (idx->bytes) {
    if ((rc = fill(idx)) != SVS_OK) {
      index_destroy(idx);
      return rc;
    }
    shadow_ingest(idx, 0, n, n, nullptr, true);
  }
  *out = idx;
  return SVS_OK;
}

// svs_index_append / _from_device behind their argument checks: copy(row0) brings the n_new rows in at row0
template <class Copy>
int append_rows(svs_index* idx, int64_t n_new, const char* what, Copy copy) {
  std::unique_lock<std::shared_mutex> geo(idx->rw);   // no search is enqueuing while the geometry changes
  HIP_TRY(hipSetDevice(idx->device));
  const int64_t n_old = idx->n, n_tot = n_old + n_new;
  int rc = ensure_capacity(idx, n_tot, false);
  if (rc != SVS_OK) return rc;
  hipError_t e = copy(n_old);
  if (e != hipSuccess) return fail(SVS_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
  shadow_ingest(idx, n_old, n_new, n_tot, nullptr, true);
  idx->n = n_tot;
  idx->dead_flag.resize((size_t)n_tot, 0);
  return sync_dead_bits(idx);
}

// ---- in-place compaction (compact.h) ----------------------------------------------------------------
// One launch of a step: destinations [dst0, dst0 + count) of `to` from `from` (gather == true: `from` is the corpus,
// read at the rows the dead list gives; false: `from` is the bounce buffer, row t for destination dst0 + t).
template <int FORM>
void launch_compact_move(const svs_index* idx, bool gather, CompactBufs from, CompactBufs to, const uint32_t* dead, int64_t ndead,
                         int64_t dst0, int64_t count, int chunks, int shadow_chunks) {
  int lanes_log2 = 0;
  while (lanes_log2 < 6 && (1 << lanes_log2) < chunks) ++lanes_log2;   // lanes per row: a power of two, a wave at most
  // destinations per wave and batch: 64 while such batches still fill the device, fewer for a short step; at least the
  // rows a wave copies at a time
  int batch_log2 = 6;
  while (batch_log2 > 6 - lanes_log2 && (count >> batch_log2) < (int64_t)idx->cu_count * 32) --batch_log2;
  const int64_t batches = (count + (1 << batch_log2) - 1) >> batch_log2;
  const int64_t blocks = std::min<int64_t>((batches + 3) / 4, (int64_t)idx->cu_count * 8);
  if (gather)
    hipLaunchKernelGGL((compact_move_kernel<FORM, true>), dim3((unsigned)blocks), dim3(256), 0, nullptr, from, to, dead, ndead, dst0, count,
                       chunks, shadow_chunks, lanes_log2, batch_log2);
  else
    hipLaunchKernelGGL((compact_move_kernel<FORM, false>), dim3((unsigned)blocks), dim3(256), 0, nullptr, from, to, dead, ndead, dst0, count,
                       chunks, shadow_chunks, lanes_log2, batch_log2);
}

void launch_compact_move(const svs_index* idx, int form, bool gather, CompactBufs from, CompactBufs to, const uint32_t* dead,
                         int64_t ndead, int64_t dst0, int64_t count, int chunks, int shadow_chunks) {
  if (form == COMPACT_SCALES) launch_compact_move<COMPACT_SCALES>(idx, gather, from, to, dead, ndead, dst0, count, chunks, shadow_chunks);
  else if (form == COMPACT_SHADOW) launch_compact_move<COMPACT_SHADOW>(idx, gather, from, to, dead, ndead, dst0, count, chunks, shadow_chunks);
  else launch_compact_move<COMPACT_PLAIN>(idx, gather, from, to, dead, ndead, dst0, count, chunks, shadow_chunks);
}

// svs_index_compact / svs_internal_compact.  bounce_rows <= 0: the default, about 32 MiB of rows.  Everything that can
// fail for want of an argument, of capacity or of memory comes before the first move.
int compact_index(svs_index* idx, int64_t bounce_rows, int64_t* out_old_rows, int64_t out_capacity, int64_t* out_n, int64_t* stats) {
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::unique_lock<std::shared_mutex> geo(idx->rw);   // no search is enqueuing while the rows move
  const int64_t n = idx->n, ndead = (int64_t)idx->dead_list.size(), n_live = n - ndead;
  if (out_n) *out_n = n_live;
  if (out_old_rows && out_capacity < n_live)
    return fail(SVS_ERR_INVALID, "svs_index_compact: %lld live rows, the row map holds %lld", (long long)n_live, (long long)out_capacity);
  if (ndead == 0) {
    for (int64_t p = 0; out_old_rows && p < n; ++p) out_old_rows[p] = idx->row_offset + p;
    return SVS_OK;
  }
  HIP_TRY(hipSetDevice(idx->device));
  int rc = staging_wait(idx);
  if (rc != SVS_OK) return rc;
  // the dead rows ascending (mask_rows appends them in the caller's order): one pass over the flags, no sort
  std::vector<uint32_t> dead((size_t)ndead + 1);
  {
    size_t j = 0;
    for (int64_t r = 0; r < n; ++r) {
      dead[j] = (uint32_t)r;
      j += idx->dead_flag[(size_t)r] != 0;
    }
    dead.resize((size_t)ndead);
  }
  const bool shadow = idx->shadow != nullptr;
  const int form = idx->row_scales ? COMPACT_SCALES : (shadow ? COMPACT_SHADOW : COMPACT_PLAIN);
  const size_t row_b = (size_t)idx->ld * elem_bytes(idx), shadow_b = shadow ? (size_t)idx->ld * sizeof(_Float16) : 0;
  const size_t scale_b = idx->row_scales ? sizeof(float) : 0;
  const int chunks = (int)(row_b / 16), shadow_chunks = (int)(shadow_b / 16);
  if (bounce_rows <= 0) bounce_rows = (int64_t)std::max<size_t>(1, ((size_t)32 << 20) / std::max<size_t>(row_b, 1));
  // plan, then the bounce buffer the plan needs; if HBM has no room for it, a smaller one and a new plan
  DevTmp tmp;
  std::vector<int64_t> steps;
  char* bounce = nullptr;
  for (;; bounce_rows /= 2) {
    if (row_b == 0) break;   // (a zero-dimensional index: nothing to move)
    const int64_t ns = compact_plan(dead.data(), ndead, n, bounce_rows, nullptr, 0);
    if (ns < 0) return fail(SVS_ERR_INVALID, "internal: bad tombstone list");
    steps.assign((size_t)ns * 3, 0);
    (void)compact_plan(dead.data(), ndead, n, bounce_rows, steps.data(), ns);
    bool bounces = false;
    for (int64_t i = 0; i < ns; ++i) bounces = bounces || steps[3 * i] == COMPACT_BOUNCE;
    if (!bounces || hipMalloc((void**)&bounce, (size_t)bounce_rows * (row_b + shadow_b + scale_b)) == hipSuccess) break;
    (void)hipGetLastError();
    bounce = nullptr;
    if (bounce_rows == 1) return fail(SVS_ERR_NOMEM, "svs_index_compact: no HBM for a bounce buffer of one row");
  }
  if (bounce) tmp.p.push_back(bounce);
  uint32_t* dead_sorted = nullptr;
  if (!steps.empty()) {
    HIP_TRY(tmp.alloc(&dead_sorted, (size_t)ndead * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(dead_sorted, dead.data(), (size_t)ndead * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  // The label column moves with the rows, OUT OF PLACE: the fresh column (and the filter's counts) are allocated here,
  // before the first row moves -- SVS_ERR_NOMEM leaves the handle untouched -- and swapped in after the rows' move
  // Every column the index owns (svs_index_set_column) moves the same way, each into its own fresh buffer.
  uint32_t *col_new[SVS_COLUMNS_MAX] = {}, *lab_cnt = nullptr;
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {
    if (!idx->cols[c]) continue;
    HIP_TRY(tmp.alloc(&col_new[c], label_column_bytes(idx->cap)));
    if (!lab_cnt) HIP_TRY(tmp.alloc(&lab_cnt, (size_t)(label_strips(n) + 2) * sizeof(uint32_t)));
  }
  // work enqueued by the device entries may still read the rows; the pipelines start their rings over
  HIP_TRY(hipDeviceSynchronize());
  for (AheadPipe* p : idx->pipes) {
    std::lock_guard<std::mutex> lk(p->mu);
    HIP_TRY(pipe_drain(p));
  }
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {
    if (!col_new[c]) continue;
    // the ordered stream compaction of the column's VALUES under "row is live" (the empty set): new row p gets the value
    // of the p-th live row; the tail stays zero.  (The predicate does not read the column, so every column would count
    // the same; the scan turns the counts into bases in place, so each column counts again: launch-bound, 4 KiB of
    // counts per million rows.)
    HIP_TRY(hipMemsetAsync(col_new[c], 0, label_column_bytes(idx->cap), nullptr));
    const LabelFilter f = label_filter(idx, c, nullptr, 0, nullptr);
    launch_label_count(f, lab_cnt, nullptr);
    launch_label_write<LB_VALUES>(f, lab_cnt, col_new[c], n_live, nullptr);
  }
  const CompactBufs corpus{(uint4*)idx->rows, idx->row_scales, (uint4*)idx->shadow};
  CompactBufs bnc{};   // rows, then shadow rows, then scales: every part starts on a 16-byte boundary
  if (bounce) bnc = CompactBufs{(uint4*)bounce, (float*)(bounce + (size_t)bounce_rows * (row_b + shadow_b)), (uint4*)(bounce + (size_t)bounce_rows * row_b)};
  int64_t moved = 0, n_direct = 0, n_bounce = 0;
  for (size_t i = 0; i < steps.size(); i += 3) {
    const int64_t kind = steps[i], dst0 = steps[i + 1], count = steps[i + 2];
    const CompactBufs at{corpus.rows + (size_t)dst0 * chunks, corpus.scales ? corpus.scales + dst0 : nullptr,
                         corpus.shadow ? corpus.shadow + (size_t)dst0 * shadow_chunks : nullptr};
    if (kind == COMPACT_DIRECT) {
      launch_compact_move(idx, form, true, corpus, at, dead_sorted, ndead, dst0, count, chunks, shadow_chunks);
      ++n_direct;
    } else {
      launch_compact_move(idx, form, true, corpus, bnc, dead_sorted, ndead, dst0, count, chunks, shadow_chunks);
      launch_compact_move(idx, form, false, bnc, at, dead_sorted, ndead, dst0, count, chunks, shadow_chunks);
      ++n_bounce;
    }
    moved += count;
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess && idx->dead_bits_dev.cap) e = hipMemset(idx->dead_bits_dev, 0, idx->dead_bits_dev.cap * sizeof(uint32_t));
  if (e == hipSuccess && idx->dead_dev.cap) e = hipMemset(idx->dead_dev, 0, idx->dead_dev.cap * sizeof(uint32_t));
  if (e != hipSuccess)
    return fail(SVS_ERR_DEVICE, "svs_index_compact: %s while rows were moving; the handle is only good for svs_index_release",
                hipGetErrorString(e));
  for (int c = 0; c < SVS_COLUMNS_MAX; ++c) {   // (the rows have moved: the compacted columns take the old ones' places)
    if (!col_new[c]) continue;
    tmp.p.erase(std::find(tmp.p.begin(), tmp.p.end(), (void*)col_new[c]));
    (void)hipFree(idx->cols[c]);
    idx->cols[c] = col_new[c];
  }
  if (out_old_rows) {   // (branch-free: the slot is overwritten until a live row keeps it; the last live row is the last write inside the map)
    int64_t p = 0;
    for (int64_t r = 0; r < n && p < n_live; ++r) {
      out_old_rows[p] = idx->row_offset + r;
      p += idx->dead_flag[(size_t)r] == 0;
    }
  }
  idx->n = n_live;
  idx->dead_flag.assign((size_t)n_live, 0);
  idx->dead_list.clear();
  idx->dead_bits.clear();
  {
    std::lock_guard<std::mutex> lk(idx->pfx_mu);
    idx->pfx_n = -1;   // (the sample's rows have moved, whatever the row count says after later appends)
  }
  idx->scr_paused.store(false);
  idx->geo_epoch.fetch_add(1);
  if (stats) {
    stats[0] = n_direct; stats[1] = n_bounce; stats[2] = moved;
    stats[3] = moved * (int64_t)(row_b + shadow_b + scale_b);
  }
  return SVS_OK;
}

// ---- shared by the host-driven batched searches (search_host, svs_index_neighbors) ----------------------------------------
// A plan that failed after plan_search created its timing events keeps none of them.
void plan_abandon(svs_index* idx, SearchPlan& plan) {
  if (!plan.timed || !plan.ev.e0) return;
  std::lock_guard<std::mutex> lk(idx->mu);
  bool kept = false;
  for (auto& t : idx->evs) kept = kept || t.e0 == plan.ev.e0;
  if (!kept) ev_destroy(plan.ev);
}

// Positions per pass of the re-run; fewer where the pass's score matrix would exceed 2 GiB: 256 at 1M rows, 53 at 10M.
// (Rounds 2-3 re-ran them one by one through the single-query kernels: 0.9 ms each at 1M rows, ~1 s for a 1024-query batch
//  over a corpus sorted by similarity, against 3 ms normally; in passes of 64 the same call took 55 ms, of 256: see DESIGN 4.)
constexpr int REDO_BATCH = 256;

// The next group of overflowed positions (first result row -2; results at stride `count`) in [*q, q1): up to `max`, ascending,
// into grp.  *q ends behind the last position looked at; 0 = none is left.  No HIP in it: svs_internal_redo_groups.
int next_redo_group(const int64_t* res_rows, int count, int64_t* q, int64_t q1, int max, int64_t* grp) {
  int m = 0;
  for (; *q < q1 && m < max; ++*q)
    if (res_rows[(size_t)*q * count] == -2) grp[m++] = *q;
  return m;
}

// Positions [q0, q1) of the pinned result block whose fused candidate list overflowed (rows ordered by similarity to the
// query, so that the prefix's threshold cuts nothing): exact re-run through the MATERIALISED path, group by group, kk results
// per query.  stage(grp, m) puts the group's queries into q_buf; the search writes tmp_s / tmp_r and finish(m) enqueues what
// moves them into redo_s_pin / redo_r_pin -- tmp_s null: the search writes there itself.  *n_redo grows by the positions re-run.
template <class Stage, class Finish>
int rerun_overflowed(svs_index* idx, HostCall& fr, int64_t q0, int64_t q1, int count, int kk, const DevBuf<float>& q_buf, float* tmp_s,
                     int64_t* tmp_r, Stage stage, Finish finish, int* n_redo) {
  const int redo_max = (int)std::min<int64_t>(REDO_BATCH, std::max<int64_t>(1, ((int64_t)2 << 30) / (4 * std::max<int64_t>(idx->n, 1))));
  Ctx* c = fr.c;
  int64_t grp[REDO_BATCH];
  int rc;
  while (const int m = next_redo_group(c->out_r_pin, count, &q0, q1, redo_max, grp)) {
    *n_redo += m;
    if ((rc = c->redo_s_pin.grow((size_t)REDO_BATCH * count)) != SVS_OK || (rc = c->redo_r_pin.grow((size_t)REDO_BATCH * count)) != SVS_OK) return rc;
    const hipStream_t st = fr.stream();   // (asked for per group: each one ends in a wait)
    if ((rc = stage(grp, m)) != SVS_OK) return rc;
    if ((rc = enqueue_search(idx, c, q_buf, m, kk, kk, tmp_s ? tmp_s : c->redo_s_pin.p, tmp_s ? tmp_r : c->redo_r_pin.p, st, false)) != SVS_OK) return rc;
    finish(m);
    if ((rc = fr.close("search", true)) != SVS_OK) return rc;
    for (int j = 0; j < m; ++j) {
      memcpy(c->out_s_pin + (size_t)grp[j] * count, c->redo_s_pin + (size_t)j * count, (size_t)count * sizeof(float));
      memcpy(c->out_r_pin + (size_t)grp[j] * count, c->redo_r_pin + (size_t)j * count, (size_t)count * sizeof(int64_t));
    }
  }
  return SVS_OK;
}

// nq results of `count` entries each (stride `count`) into the caller's block (stride k >= count).  counts (may be null):
// the results are ragged, query qi has counts[qi] <= count entries (below 1: none)
template <class T>
void deliver_strided(T* dst, int k, const T* src, int count, int64_t nq, const int32_t* counts = nullptr) {
  if (count == k && !counts) {   // (one piece)
    memcpy(dst, src, (size_t)nq * count * sizeof(T));
    return;
  }
  for (int64_t qi = 0; qi < nq; ++qi) {
    const int c = counts ? counts[qi] : count;
    if (c > 0) memcpy(dst + (size_t)qi * k, src + (size_t)qi * count, (size_t)c * sizeof(T));
  }
}

// The pinned result block into the caller's
void deliver_results(const Ctx* c, int64_t nq, int count, int k, float* out_scores, int64_t* out_rows) {
  deliver_strided(out_scores, k, c->out_s_pin.p, count, nq);
  deliver_strided(out_rows, k, c->out_r_pin.p, count, nq);
}

// A caller's list of global rows: every one a row of an index of n rows from row `lo`.  *ascending (may be null):
// strictly, so that the list needs neither sorting nor deduplication.
int check_row_list(const int64_t* rows, int64_t nrows, int64_t lo, int64_t n, bool* ascending) {
  if (nrows < 0) return fail(SVS_ERR_INVALID, "nrows must be >= 0");
  if (nrows > 0 && !rows) return fail(SVS_ERR_INVALID, "null row list");
  if (ascending) *ascending = true;
  for (int64_t t = 0; t < nrows; ++t) {
    const int64_t r = rows[t] - lo;
    if (r < 0 || r >= n)
      return fail(SVS_ERR_INVALID, "row %lld out of range [%lld, %lld)", (long long)rows[t], (long long)lo, (long long)(lo + n));
    if (ascending && t && rows[t] <= rows[t - 1]) *ascending = false;
  }
  return SVS_OK;
}

// The live rows of a checked list of global rows, as local u32 rows, ascending and without repeats, into dst (room for
// nrows); returns how many.  ascending: the list is strictly so already (check_row_list) and is filtered as it stands;
// otherwise it is sorted in tmp first, which may throw std::bad_alloc.  No HIP in it: svs_internal_live_rows.
int64_t live_rows_ascending(const int64_t* rows, int64_t nrows, int64_t lo, const uint8_t* dead_flag, bool ascending,
                            std::vector<uint32_t>& tmp, uint32_t* dst) {
  int64_t m = 0;
  if (ascending) {
    for (int64_t t = 0; t < nrows; ++t) {
      const uint32_t r = (uint32_t)(rows[t] - lo);
      if (!dead_flag[r]) dst[m++] = r;
    }
    return m;
  }
  tmp.resize((size_t)nrows);
  for (int64_t t = 0; t < nrows; ++t) tmp[(size_t)t] = (uint32_t)(rows[t] - lo);
  std::sort(tmp.begin(), tmp.end());
  const size_t u = (size_t)(std::unique(tmp.begin(), tmp.end()) - tmp.begin());
  for (size_t t = 0; t < u; ++t)
    if (!dead_flag[tmp[t]]) dst[m++] = tmp[t];
  return m;
}

// The call's qn query floats: caller -> pinned staging -> c->q_dev, one copy each
int upload_queries(Ctx* c, const float* queries, size_t qn, hipStream_t st) {
  int rc;
  if ((rc = c->q_dev.grow(qn)) != SVS_OK || (rc = c->q_pin.grow(qn)) != SVS_OK) return rc;
  memcpy(c->q_pin, queries, qn * sizeof(float));
  HIP_TRY(hipMemcpyAsync(c->q_dev, c->q_pin, qn * sizeof(float), hipMemcpyHostToDevice, st));
  return SVS_OK;
}

// ---- svs_index_assign, svs_index_label_sums: the timing hooks' readings, -1 from the moment a call of the entry begins
// until that call has timed its kernels (TimedSpan); a call of the other entry never touches it
thread_local double g_assign_kernel_ms = -1.0;       // svs_internal_assign_kernel_ms
thread_local double g_label_sums_kernel_ms = -1.0;   // svs_internal_label_sums_kernel_ms
thread_local double g_collapse_ms[4] = {-1.0, -1.0, -1.0, -1.0};   // svs_internal_collapse_kernel_ms: reduce, mark, clear, select
thread_local double g_collapsed_combined_ms[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};   // svs_internal_collapsed_combined_kernel_ms: scores, reduce, mark, clear, select
thread_local double g_collapse_scope_ms[6] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0};   // svs_internal_collapse_scope_kernel_ms: filter, gather, reduce, mark, clear, select
thread_local double g_score_pass_ms = -1.0;         // svs_internal_score_pass_ms: the score pass of the last combined_scores / multi_scores hook call
int report_ms(double* out, double ms) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  *out = ms;
  return SVS_OK;
}

// accumulators per wave: one sweep of 64 vectors covers a small c, 256 per sweep beyond
template <int DT, int NA>
void launch_assign_na(const svs_index* idx, const Ctx* cx, int c, int64_t r0, int64_t nrows, const uint32_t* vec_labels, int32_t* best,
                             float* scores, uint32_t* labels, unsigned long long* counts, hipStream_t st) {
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  const unsigned blocks = (unsigned)std::min<int64_t>((nrows + AS_ROWS - 1) / AS_ROWS, AS_GRID_MAX);
  hipLaunchKernelGGL((assign_rows_kernel<DT, NA>), dim3(blocks), dim3(AS_THREADS), 0, st, (const u32x4*)idx->rows, ld16,
                     (const float*)idx->row_scales, idx->n, (const u32x4*)cx->as_vec.p, (const float*)cx->as_vec_scales.p, c, r0, nrows,
                     dead_bits_of(idx), vec_labels, best, scores, labels, counts);
}

// The context's one score vector over all n rows: the tombstoned rows' scores go to -inf, then the exact top-k stage
// writes the best `count` rows (global) to out_s / out_r
int select_live(svs_index* idx, Ctx* c, int count, float* out_s, int64_t* out_r, hipStream_t st) {
  const int64_t n = idx->n, sstride = score_stride(n);
  if (!idx->dead_list.empty())
    hipLaunchKernelGGL(mask_dead_rows_kernel, dim3(64), dim3(256), 0, st, c->scores.p, sstride, 1, (const uint32_t*)idx->dead_dev.p,
                       (int64_t)idx->dead_list.size(), n, (int64_t)0);
  return run_select(idx, c, c->scores, n, sstride, 1, count, count, out_s, out_r, st, idx->row_offset);
}

// ---- the filtered searches: svs_index_search_labeled (labels.h) and svs_index_search_where (where.h)
// Every successful exit of the two: the entries written, the rows that matched
int32_t filtered_done(int32_t* out_count, int64_t* out_matched, int count, int64_t m) {
  if (out_count) *out_count = count;
  if (out_matched) *out_matched = m;
  return SVS_OK;
}

struct FilteredNames {
  const char *entry, *count_kernel, *write_kernel;   // the entry's short name for the messages, the two recorded launches
};

// What the two do once their arguments are checked (the caller holds the index's shared lock): plan (a LabelSet or a
// WherePlan) stages its filter, the strips are counted, and the matching rows' list is written and searched on the
// device.  record_arg: the recorded launches' second figure; ranks: results are wanted, if a row matches.
template <class PLAN>
int32_t filtered_search(svs_index* idx, const PLAN& plan, const FilteredNames& names, int record_arg, bool ranks, const float* queries,
                               int32_t nq, int32_t d, int32_t k, float* out_scores, int64_t* out_rows, int32_t* out_count, int64_t* out_matched) {
  if (!ranks && !out_matched) return filtered_done(out_count, out_matched, 0, 0);   // nothing to rank and nobody to tell the count
  int rc;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const int64_t n = idx->n, lo = idx->row_offset;
  if ((rc = c->lab_cnt.grow((size_t)label_strips(n) + 2)) != SVS_OK || (rc = c->lab_tot_pin.grow(1)) != SVS_OK) return rc;
  // 1. the filter goes up, the count runs; the host needs m = |S| to size the list, the score matrix and the select route
  hipStream_t st = fr.stream();
  typename PLAN::Filter f;
  if ((rc = plan.stage(idx, c, st, &f)) != SVS_OK) return rc;
  launch_record(names.count_kernel, n, record_arg);
  launch_label_count(f, c->lab_cnt, st);
  HIP_TRY(hipMemcpyAsync(c->lab_tot_pin, c->lab_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  if ((rc = fr.close(names.entry)) != SVS_OK) return rc;
  const int64_t m = (int64_t)c->lab_tot_pin[0];
  if (m < 0 || m > n) return fail(SVS_ERR_DEVICE, "%s: the filter counted %lld of %lld rows", names.entry, (long long)m, (long long)n);
  const int count = ranks ? (int)std::min<int64_t>(k, m) : 0;
  if (count == 0) return filtered_done(out_count, out_matched, 0, m);
  // 2. the list is written on the device; from here on the call is svs_index_search_rows over it
  const size_t qn = (size_t)nq * (size_t)d, on = (size_t)nq * (size_t)count;
  if ((rc = c->list_dev.grow((size_t)m)) != SVS_OK || (rc = c->lab_pos.grow(on)) != SVS_OK) return rc;
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  st = fr.stream();
  if ((rc = upload_queries(c, queries, qn, st)) != SVS_OK) return rc;
  launch_record(names.write_kernel, n, record_arg);
  launch_label_write<LB_ROWS>(f, c->lab_cnt, c->list_dev, m, st);
  if ((rc = search_list_chunked(idx, c, nq, d, c->list_dev, m, count, c->out_s_pin, c->lab_pos, st)) != SVS_OK) return rc;
  // the positions -> global rows, on the device: the list never exists on the host
  hipLaunchKernelGGL(label_map_rows_kernel, dim3((unsigned)std::min<size_t>((on + 255) / 256, 1024)), dim3(256), 0, st,
                     (const int64_t*)c->lab_pos.p, (int64_t)on, (const uint32_t*)c->list_dev.p, m, lo, c->out_r_pin.p);
  if ((rc = fr.close(names.entry)) != SVS_OK) return rc;
  for (size_t i = 0; i < on; ++i)
    if (c->out_r_pin[i] < 0)
      return fail(SVS_ERR_DEVICE, "%s: result %zu of query %zu is a position outside the %lld matching rows", names.entry, i % (size_t)count,
                  i / (size_t)count, (long long)m);
  deliver_results(c, nq, count, k, out_scores, out_rows);
  return filtered_done(out_count, out_matched, count, m);
}

}  // namespace

extern "C" {

const char* svs_version(void) { return "svs_amd 0.3.0 (gfx950)"; }
const char* svs_last_error(void) { return g_err.c_str(); }
// (multi.hip: carries a worker thread's message over to the caller's thread; not part of the ABI)
int32_t svs_internal_set_error(int32_t code, const char* msg) { return fail(code, "%s", msg ? msg : ""); }

int32_t svs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t svs_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes) {
  HIP_TRY(hipSetDevice(device));
  size_t f = 0, t = 0;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return SVS_OK;
}

int32_t svs_index_create(const float* host_rows, int64_t n, int32_t d, int32_t store_dtype,
                         int32_t device, int64_t row_offset, svs_index** out) {
  return create_index(n, d, store_dtype, device, row_offset, out, [&](svs_index* idx) {
    if (!host_rows) return fail(SVS_ERR_INVALID, "null host_rows");
    hipError_t e = upload_host_rows(idx, host_rows, n, 0);
    return e == hipSuccess ? (int)SVS_OK : fail(SVS_ERR_DEVICE, "corpus upload: %s", hipGetErrorString(e));
  });
}

int32_t svs_index_create_from_device(const float* dev_rows, int64_t n, int32_t d, int64_t src_ld,
                                     int32_t store_dtype, int32_t device, int64_t row_offset,
                                     svs_index** out) {
  return create_index(n, d, store_dtype, device, row_offset, out, [&](svs_index* idx) {
    if (!dev_rows || src_ld < d) return fail(SVS_ERR_INVALID, "bad device source (ptr %p, ld %lld)", (const void*)dev_rows, (long long)src_ld);
    hipError_t e = copy_device_rows(idx, dev_rows, n, src_ld, 0);
    return e == hipSuccess ? (int)SVS_OK : fail(SVS_ERR_DEVICE, "device corpus copy: %s", hipGetErrorString(e));
  });
}

int32_t svs_index_append(svs_index* idx, const float* host_rows, int64_t n_new) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (n_new < 0) return fail(SVS_ERR_INVALID, "negative row count");
  if (n_new == 0) return SVS_OK;
  if (!host_rows) return fail(SVS_ERR_INVALID, "null host_rows");
  if (idx->d == 0) return fail(SVS_ERR_SHAPE, "cannot append to a zero-dimensional index");
  return append_rows(idx, n_new, "append upload", [&](int64_t row0) { return upload_host_rows(idx, host_rows, n_new, row0); });
}

int32_t svs_index_reserve(svs_index* idx, int64_t rows_capacity) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (idx->d == 0) return fail(SVS_ERR_SHAPE, "cannot reserve rows of a zero-dimensional index");
  std::unique_lock<std::shared_mutex> geo(idx->rw);
  HIP_TRY(hipSetDevice(idx->device));
  idx->geo_epoch.fetch_add(1);
  return ensure_capacity(idx, rows_capacity, true);
}

int32_t svs_index_append_from_device(svs_index* idx, const float* dev_rows, int64_t n_new, int64_t src_ld) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (n_new < 0) return fail(SVS_ERR_INVALID, "negative row count");
  if (n_new == 0) return SVS_OK;
  if (idx->d == 0) return fail(SVS_ERR_SHAPE, "cannot append to a zero-dimensional index");
  if (!dev_rows || src_ld < idx->d) return fail(SVS_ERR_INVALID, "bad device source (ptr %p, ld %lld)", (const void*)dev_rows, (long long)src_ld);
  return append_rows(idx, n_new, "device append", [&](int64_t row0) { return copy_device_rows(idx, dev_rows, n_new, src_ld, row0); });
}

int32_t svs_index_staging_acquire(svs_index* idx, float** host_block, int64_t* rows_cap) {
  if (!idx || !host_block || !rows_cap) return fail(SVS_ERR_INVALID, "null argument");
  if (idx->d == 0) return fail(SVS_ERR_SHAPE, "cannot stage rows of a zero-dimensional index");
  HIP_TRY(hipSetDevice(idx->device));
  std::lock_guard<std::mutex> lk(idx->stg_mu);
  auto& g = idx->stg;
  if (!g.active) {
    const size_t row_b = (size_t)idx->d * sizeof(float);
    g.rows_cap = (int64_t)std::max<size_t>(1, ((size_t)32 << 20) / row_b);
    // (a failure half way through the first-time set-up must not strand the stream and the blocks made so far:
    //  the next acquire would make them again)
    hipError_t e = hipStreamCreateWithFlags(&g.st, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
      e = hipHostMalloc(&g.pin[i], (size_t)g.rows_cap * row_b, hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&g.done[i], hipEventDisableTiming);
      if (e == hipSuccess && idx->dtype != SVS_DTYPE_F32) e = hipMalloc((void**)&g.dstage[i], (size_t)g.rows_cap * row_b);
    }
    if (e != hipSuccess) {
      staging_free(idx);
      return fail(e == hipErrorOutOfMemory ? SVS_ERR_NOMEM : SVS_ERR_DEVICE, "staging blocks: %s", hipGetErrorString(e));
    }
    g.cur = 1;
    g.active = true;
  }
  g.cur ^= 1;
  HIP_TRY(hipEventSynchronize(g.done[g.cur]));   // the DMA that last read this block (never recorded: returns at once)
  *host_block = (float*)g.pin[g.cur];
  *rows_cap = g.rows_cap;
  return SVS_OK;
}

int32_t svs_index_staging_commit(svs_index* idx, int64_t n_rows) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (n_rows < 0) return fail(SVS_ERR_INVALID, "negative row count");
  if (n_rows == 0) return SVS_OK;
  std::unique_lock<std::shared_mutex> geo(idx->rw);
  std::lock_guard<std::mutex> lk(idx->stg_mu);
  auto& g = idx->stg;
  if (!g.active) return fail(SVS_ERR_INVALID, "svs_index_staging_commit without svs_index_staging_acquire");
  if (n_rows > g.rows_cap) return fail(SVS_ERR_INVALID, "%lld rows do not fit the staging block (%lld)", (long long)n_rows, (long long)g.rows_cap);
  HIP_TRY(hipSetDevice(idx->device));
  const int64_t n_old = idx->n, n_tot = n_old + n_rows;
  if (n_tot > idx->cap) {   // growing reallocates: drain our own copies first (ensure_capacity drains the rest)
    HIP_TRY(hipStreamSynchronize(g.st));
    int rc = ensure_capacity(idx, n_tot, false);
    if (rc != SVS_OK) return rc;
  }
  const int d = idx->d, b = g.cur;
  if (idx->dtype != SVS_DTYPE_F32)
    HIP_TRY(hipMemcpyAsync(g.dstage[b], g.pin[b], (size_t)n_rows * d * sizeof(float), hipMemcpyHostToDevice, g.st));
  else if (idx->ld != d)
    HIP_TRY(hipMemsetAsync((float*)idx->rows + (size_t)n_old * idx->ld, 0, (size_t)n_rows * idx->ld * sizeof(float), g.st));
  HIP_TRY(ingest_rows(idx, idx->dtype != SVS_DTYPE_F32 ? g.dstage[b] : (const float*)g.pin[b], n_rows, d, n_old, hipMemcpyHostToDevice, 2048, g.st));
  shadow_ingest(idx, n_old, n_rows, n_tot, g.st, false);   // (on the staging stream, behind the DMA it reads)
  HIP_TRY(hipEventRecord(g.done[b], g.st));
  idx->staging_pending.store(true);
  idx->n = n_tot;
  idx->dead_flag.resize((size_t)n_tot, 0);
  return sync_dead_bits(idx);
}

int32_t svs_index_staging_finish(svs_index* idx) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  HIP_TRY(hipSetDevice(idx->device));
  std::lock_guard<std::mutex> lk(idx->stg_mu);
  if (idx->stg.st) HIP_TRY(hipStreamSynchronize(idx->stg.st));
  shadow_refresh_stats(idx);
  staging_free(idx);
  return SVS_OK;
}

int32_t svs_index_mask_rows(svs_index* idx, const int64_t* rows, int64_t count) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (count < 0 || (count > 0 && !rows)) return fail(SVS_ERR_INVALID, "bad row list");
  std::unique_lock<std::shared_mutex> geo(idx->rw);
  for (int64_t t = 0; t < count; ++t) {
    const int64_t r = rows[t] - idx->row_offset;
    if (r < 0 || r >= idx->n) return fail(SVS_ERR_INVALID, "row %lld out of range", (long long)rows[t]);
  }
  bool changed = false;
  for (int64_t t = 0; t < count; ++t) {
    const int64_t r = rows[t] - idx->row_offset;
    if (!idx->dead_flag[(size_t)r]) {
      idx->dead_flag[(size_t)r] = 1;
      idx->dead_list.push_back((uint32_t)r);
      changed = true;
    }
  }
  if (!changed) return SVS_OK;
  idx->geo_epoch.fetch_add(1);
  HIP_TRY(hipSetDevice(idx->device));
  {
    int rc = sync_dead_bits(idx);
    if (rc != SVS_OK) return rc;
  }
  if (idx->dead_list.size() > idx->dead_dev.cap) {
    int rc = grow_drained(idx->dead_dev, idx->dead_list.size() * 2 + 64);
    if (rc != SVS_OK) return rc;
  }
  HIP_TRY(hipMemcpy(idx->dead_dev, idx->dead_list.data(), idx->dead_list.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return SVS_OK;
}

int32_t svs_index_compact(svs_index* idx, int64_t* out_old_rows, int64_t out_capacity, int64_t* out_n) {
  return compact_index(idx, 0, out_old_rows, out_capacity, out_n, nullptr);
}

int32_t svs_internal_compact(svs_index* idx, int64_t bounce_rows, int64_t* out_old_rows, int64_t cap, int64_t* out_n, int64_t* stats) {
  return compact_index(idx, bounce_rows, out_old_rows, cap, out_n, stats);
}

int64_t svs_internal_compact_plan(const uint32_t* dead_sorted, int64_t ndead, int64_t n, int64_t bounce_rows, int64_t* steps, int64_t cap) {
  const int64_t ns = compact_plan(dead_sorted, ndead, n, bounce_rows, steps, cap);
  if (ns < 0) return fail(SVS_ERR_INVALID, "svs_internal_compact_plan: the dead rows must ascend strictly inside [0, n), bounce_rows >= 1");
  return ns;
}

int64_t svs_internal_segments_plan(const int64_t* sizes, const int32_t* seg_query, int64_t nseg, int32_t w, int64_t* tiles, int64_t cap,
                                   int64_t* seg_off, int64_t* total_rows) {
  if (nseg < 0 || w < 1 || cap < 0 || (nseg > 0 && !sizes) || (cap > 0 && !tiles))
    return fail(SVS_ERR_INVALID, "svs_internal_segments_plan: nseg >= 0, w >= 1, cap >= 0");
  for (int64_t s = 0; s < nseg; ++s)
    if (sizes[s] < 0) return fail(SVS_ERR_INVALID, "svs_internal_segments_plan: segment %lld has a negative size", (long long)s);
  const int64_t nt = seg_tile_plan(sizes, seg_query, nseg, w, nullptr, 0, seg_off, total_rows);
  if (nt < 0) return fail(SVS_ERR_UNSUPPORTED, "svs_internal_segments_plan: 2^31 or more live rows in the small segments");
  const int64_t keep = std::min(nt, cap);
  if (keep > 0) {
    std::vector<SegTile> t;
    try {
      t.resize((size_t)keep);
    } catch (const std::bad_alloc&) {
      return fail(SVS_ERR_NOMEM, "out of host memory for %lld tiles", (long long)keep);
    }
    (void)seg_tile_plan(sizes, seg_query, nseg, w, t.data(), keep, nullptr, nullptr);
    for (int64_t i = 0; i < keep; ++i) {
      tiles[4 * i] = t[(size_t)i].off;
      tiles[4 * i + 1] = t[(size_t)i].rows;
      tiles[4 * i + 2] = t[(size_t)i].query;
      tiles[4 * i + 3] = t[(size_t)i].seg;
    }
  }
  return nt;
}

int32_t svs_index_retain(svs_index* idx) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  idx->refs.fetch_add(1);
  return SVS_OK;
}

int32_t svs_index_release(svs_index* idx) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (idx->refs.fetch_sub(1) == 1) index_destroy(idx);
  return SVS_OK;
}

int32_t svs_index_info(const svs_index* idx, svs_index_info_t* out) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  out->n = idx->n;
  out->d = idx->d;
  out->ld = idx->ld;
  out->dtype = idx->dtype;
  out->device = idx->device;
  out->row_offset = idx->row_offset;
  out->hbm_bytes = (int64_t)(idx->bytes + idx->shadow_bytes + idx->cols_bytes());
  out->n_masked = (int64_t)idx->dead_list.size();
  return SVS_OK;
}

// The host search inside an open frame, under the caller's reference and geometry lock: nq >= 1 checked queries, count
// (1 .. live rows) results each.  They end up in the context's pinned block c->out_s_pin / c->out_r_pin at stride count
// (device-visible), and from there in out_scores / out_rows at stride k -- unless out_scores is null: the caller
// (svs_index_search_diverse) goes on from the pinned block.
static int32_t search_host_framed(svs_index* idx, HostCall& fr, const float* queries, int32_t nq, int32_t d, int32_t k, int count,
                                  float* out_scores, int64_t* out_rows) {
  int rc;
  Ctx* const c = fr.c;
  const size_t qn = (size_t)nq * (size_t)d, on = (size_t)nq * (size_t)count;
  if ((rc = c->q_dev.grow(qn)) != SVS_OK) return rc;
  if ((rc = c->q_pin.grow(qn)) != SVS_OK) return rc;
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  const hipStream_t st = fr.stream();
  // The final top-k kernel stores its k results straight into the pinned host
  // buffers (device-visible, zero-copy): no D2H copies on the latency path.
  const auto t_begin = std::chrono::steady_clock::now();
  auto stamp = [&](int i) { g_host_phase[i] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
  SearchPlan plan;
  if ((rc = plan_search(idx, c, nq, count, count, st, true, idx->variant.load(), &plan)) != SVS_OK) return rc;
  stamp(0);
  const int64_t mode = g_tune_upload.load();
  // f16 batches: the staging kernel (convert_queries_f16) reads the f32 queries STRAIGHT out of the pinned buffer, over PCIe,
  // once, and writes the half image the GEMM kernels use -- no copy-engine transfer, no f32 copy of the queries in HBM, no
  // hand-over between the DMA engine and the compute queue in front of the first kernel -- CHUNK BY CHUNK (<= 1 MiB of whole
  // queries): chunk j is pulled over the bus while the host copies chunk j + 1 into pinned memory.  Measured on configs[2]
  // (6.3 MB of queries; tools/call_breakdown.py): 0.088 ms until everything is enqueued against 0.15 with the DMA calls in
  // between.  f32 indexes keep the staged DMA (their kernels read the f32 queries themselves, many times), and so do fp8
  // ones: quantize_rows_fp8 reads its source twice -- row maximum, then the bytes -- and over the bus that cost configs[4]
  // 0.03-0.05 ms per call.  (Also measured and dropped: helper threads sharing the host copy -- their hand-offs cost what
  // they saved, 0.112 vs 0.088 ms to fill the pinned buffer; and the prefix pass per query tile, see SearchPlan.)
  const bool pull = mode == 0 && plan.batch.query == BatchRoute::HALF;
  const float* q_src = pull ? c->q_pin.p : c->q_dev.p;
  if (pull) {
    const int rows_total = plan.batch.rows();               // the image of the WHOLE batch: sized once, before the first chunk
    rc = c->qh.grow((size_t)rows_total * idx->ld);
    int cq = 256;                                           // queries per chunk: <= 1 MiB, a power of two
    while (cq > 1 && (size_t)cq * d * sizeof(float) > ((size_t)1 << 20)) cq >>= 1;
    for (int q0 = 0; q0 < nq && rc == SVS_OK; q0 += cq) {
      const int nc = std::min(cq, nq - q0);
      const size_t off = (size_t)q0 * d;
      memcpy(c->q_pin + off, queries + off, (size_t)nc * d * sizeof(float));
      // (rows [q0, q0 + nc) of the image; the last chunk also zeroes the padding rows behind the batch)
      rc = stage_queries_f16(idx, c, c->q_pin + off, nc, q0 + nc == nq ? rows_total : q0 + nc, st, q0);
    }
    plan.q_staged = c->qh.p;
  } else {
    // queries -> pinned staging -> HBM, in 1 MiB pieces: the DMA of piece i runs under the host copy of piece i + 1
    for (size_t off = 0; off < qn; off += (size_t)262144) {
      const size_t len = std::min((size_t)262144, qn - off);
      memcpy(c->q_pin + off, queries + off, len * sizeof(float));
      HIP_TRY(hipMemcpyAsync(c->q_dev + off, c->q_pin + off, len * sizeof(float), hipMemcpyHostToDevice, st));
    }
  }
  stamp(1);
  if (rc == SVS_OK) rc = enqueue_prefix(idx, c, plan, q_src, st);
  if (rc == SVS_OK) rc = enqueue_main(idx, c, plan, q_src, c->out_s_pin, c->out_r_pin, st);
  stamp(2);
  if (rc == SVS_OK) rc = fr.wait();
  if (rc != SVS_OK) {
    plan_abandon(idx, plan);
    return rc;
  }
  stamp(3);
  // The group's queries go to the front of q_dev in ONE copy -- whatever the main pass kept there is no longer needed, the
  // pinned buffer still holds every query of the call; a group that is not one run of queries is gathered first.
  auto stage = [&](const int64_t* grp, int m) -> int {
    const float* src = c->q_pin + (size_t)grp[0] * d;
    if (grp[m - 1] - grp[0] != m - 1) {
      if (int rc = c->redo_q_pin.grow((size_t)REDO_BATCH * d); rc != SVS_OK) return rc;
      for (int j = 0; j < m; ++j) memcpy(c->redo_q_pin + (size_t)j * d, c->q_pin + (size_t)grp[j] * d, (size_t)d * sizeof(float));
      src = c->redo_q_pin;
    }
    HIP_TRY(hipMemcpyAsync(c->q_dev, src, (size_t)m * d * sizeof(float), hipMemcpyHostToDevice, st));
    return SVS_OK;
  };
  int n_redo = 0;
  if ((rc = rerun_overflowed(idx, fr, 0, nq, count, count, c->q_dev, nullptr, nullptr, stage, [](int) {}, &n_redo)) != SVS_OK) return rc;
  g_host_phase[5] = (double)n_redo;   // (svs_internal_host_phases: queries of this call that were re-run)
  if (out_scores) deliver_results(c, nq, count, k, out_scores, out_rows);
  stamp(4);
  return SVS_OK;
}

static int32_t search_host(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                           float* out_scores, int64_t* out_rows, int32_t* out_count) {
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  const int count = (int)std::min<int64_t>(std::max(k, 0), idx->n - (int64_t)idx->dead_list.size());
  if (out_count) *out_count = count;
  if (nq == 0 || count == 0) return SVS_OK;
  if (!out_scores || !out_rows) return fail(SVS_ERR_INVALID, "null output");
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  return search_host_framed(idx, fr, queries, nq, d, k, count, out_scores, out_rows);
}

int32_t svs_index_search(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                         float* out_scores, int64_t* out_rows, int32_t* out_count) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  // (only well-formed single queries are coalesced: every error stays with the call that made it)
  // (and only ordinary k: a "rank everything" call must not size a whole pass's buffers)
  if (!(idx->coalesce.load() && nq == 1 && k > 0 && k <= 2048 && d == idx->d && queries && out_scores && out_rows && idx->n > 0))
    return search_host(idx, queries, nq, d, k, out_scores, out_rows, out_count);
  RefGuard guard(idx);
  // f32: whole kernel tiles -- the exact-f32 MFMA kernels cost the same for 33 queries as for 64 (1.8 vs 1.2 ms
  // for 32), so a queue that does not fill the next tile size leaves its tail for the following pass.
  // f16 / fp8: the passes are HBM-bound up to 128 queries and cost almost the same whatever they carry
  // (1M x 1536 f16: 0.57 / 0.60 / 0.64 ms at 16 / 32 / 64 queries; fp8 0.32 / 0.33 / 0.40): cutting 40
  // queued callers into 32 + 8 would cost two passes for the price of one, so everything queued goes out.
  return idx->co.search(
      queries, d, k, out_scores, out_rows, out_count,
      [&](const float* q, int n, int kmax, float* s, int64_t* r, int32_t* cnt) { return search_host(idx, q, n, d, kmax, s, r, cnt); },
      [&] { return idx->co_round.load() && idx->dtype == SVS_DTYPE_F32; });
}

int32_t svs_index_set_coalesce(svs_index* idx, int32_t enable) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  idx->coalesce.store(enable != 0);
  idx->co_round.store(enable != 2);   // (2: take everything that is queued, whatever the tile sizes -- A/B)
  return SVS_OK;
}

int32_t svs_index_coalesce_stats(svs_index* idx, int64_t* passes, int64_t* queries) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (passes) *passes = idx->co.passes.load();
  if (queries) *queries = idx->co.queries.load();
  return SVS_OK;
}

// (tests and tools only -- csrc/internal.h, not in include/svs_amd.h: the NEXT coalesced pass waits, at most 5 s,
//  until n single-query calls are queued, so that a pass of a chosen size can be formed on purpose)
int32_t svs_internal_coalesce_hold(svs_index* idx, int32_t n) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (n < 0 || n > 256) return fail(SVS_ERR_INVALID, "svs_internal_coalesce_hold: 0 <= n <= 256");
  idx->co.set_hold(n);
  return SVS_OK;
}

int32_t svs_index_coalesce_sizes(svs_index* idx, int64_t* out, int32_t cap) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (!out || cap < 0 || cap > 257) return fail(SVS_ERR_INVALID, "svs_index_coalesce_sizes: out must hold cap <= 257 counters");
  for (int s = 0; s < cap; ++s) out[s] = idx->co.sizes[s].load();
  return SVS_OK;
}

// Nothing the pipeline enqueued is still running (no call is inside it either: the caller holds p->mu).  Leaves no
// "not ready" behind for a later hipGetLastError.
static bool pipe_idle(AheadPipe* p) {
  bool idle = hipStreamQuery(p->pass) == hipSuccess;
  for (int j = 0; j < AHEAD_RING && idle; ++j) idle = !p->used[j] || hipEventQuery(p->sel_done[j]) == hipSuccess;
  (void)hipGetLastError();
  return idle;
}

// The pipeline of (idx, caller), made on first use.  When kMaxPipes exist and none is this stream's, the least
// recently used one that is idle is handed over: a pipeline's stream, contexts and events serve any caller stream
// (the key only finds it again), and an idle one has no ordering left to keep.  *out stays null when every pipeline
// has work in flight: the call is then a plain one (ahead_plain counts them).
static int pipe_get(svs_index* idx, hipStream_t caller, AheadPipe** out) {
  *out = nullptr;
  std::lock_guard<std::mutex> lk(idx->mu);
  for (AheadPipe* p : idx->pipes)
    if (p->caller == caller) {
      p->tick = ++idx->pipe_tick;
      *out = p;
      return SVS_OK;
    }
  if ((int)idx->pipes.size() >= svs_index::kMaxPipes) {
    AheadPipe* pick = nullptr;
    for (AheadPipe* p : idx->pipes) {
      if (pick && p->tick >= pick->tick) continue;
      if (!p->mu.try_lock()) continue;   // (a call is enqueuing on it)
      if (pipe_idle(p)) pick = p;
      p->mu.unlock();
    }
    if (!pick) return SVS_OK;
    pick->caller = caller;
    pick->tick = ++idx->pipe_tick;
    idx->ahead_retired.fetch_add(1);
    *out = pick;
    return SVS_OK;
  }
  AheadPipe* p = new (std::nothrow) AheadPipe();
  if (!p) return fail(SVS_ERR_NOMEM, "host allocation failed");
  p->caller = caller;
  p->tick = ++idx->pipe_tick;
  p->per_pass = g_tune_handover.load() == 1;
  p->share_limit = (int)g_tune_share.load();
  hipError_t e = hipStreamCreateWithFlags(&p->pass, hipStreamNonBlocking);
  const size_t mail_bytes = sizeof(MailEntry) * MAILBOX_SIZE + sizeof(uint32_t) * SHARE_MIRROR_WORDS;
  if (e == hipSuccess) e = hipHostMalloc((void**)&p->mailbox, mail_bytes, hipHostMallocDefault);
  if (e == hipSuccess) memset(p->mailbox, 0, mail_bytes);
  else p->mailbox = nullptr;
  if (e == hipSuccess) e = hipMalloc((void**)&p->share_dev, sizeof(ShareState));
  if (e == hipSuccess) e = hipMemset(p->share_dev, 0, sizeof(ShareState));
  for (int j = 0; j < AHEAD_RING && e == hipSuccess; ++j) {
    p->ctx[j] = new (std::nothrow) Ctx();
    if (!p->ctx[j]) { e = hipErrorOutOfMemory; break; }
    p->ctx[j]->slot = svs_index::kMaxCtx + AHEAD_RING * (int)idx->pipes.size() + j;
    e = hipEventCreateWithFlags(&p->pass_done[j], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->sel_done[j], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    pipe_destroy(p);
    return fail(e == hipErrorOutOfMemory ? SVS_ERR_NOMEM : SVS_ERR_DEVICE, "run-ahead pipeline: %s", hipGetErrorString(e));
  }
  idx->pipes.push_back(p);
  *out = p;
  return SVS_OK;
}

// What a single-query search takes from its context, in elements per buffer (hist: queries): the scores, what the
// route's staging (launch_scores) and the selection path (run_select) grow.  A pipeline's contexts get it TOGETHER
// (enqueue_ahead), so those lazy grow calls are no-ops on the ring and free nothing a search in flight reads.
struct SingleScratch { size_t scores, hist, keys, q16, qh, q8, q8s, q8f; };
static SingleScratch single_scratch(const svs_index* idx, const SingleRoute& r, SelectPath sel) {
  const size_t ld = (size_t)idx->ld, half = r.query == SingleRoute::HALF, fp8 = r.query == SingleRoute::FP8;
  return {(size_t)score_stride(idx->n), sel == SelectPath::WINDOW, sel == SelectPath::SORT ? (size_t)next_pow2_i64(idx->n) : 0,
          r.query == SingleRoute::PADDED ? (size_t)GQ * ld : 0, half * ld, fp8 * ld, fp8, fp8 * ld};
}
static bool ahead_scratch_ok(const Ctx* c, const SingleScratch& s) {
  return s.scores <= c->scores.cap && s.hist <= c->hist_cap && s.keys <= c->keys.cap && s.q16 <= c->q16.cap && s.qh <= c->qh.cap &&
         s.q8 <= c->q8.cap && s.q8s <= c->q8s.cap && s.q8f <= c->q8f.cap;
}
static int ahead_scratch_grow(Ctx* c, const SingleScratch& s, hipStream_t st) {
  int rc;
  if ((rc = c->scores.grow(s.scores)) != SVS_OK || (rc = grow_select_scratch(c, (int)s.hist, st)) != SVS_OK ||
      (rc = c->keys.grow(s.keys)) != SVS_OK || (rc = c->q16.grow(s.q16)) != SVS_OK || (rc = c->qh.grow(s.qh)) != SVS_OK ||
      (rc = c->q8.grow(s.q8)) != SVS_OK || (rc = c->q8s.grow(s.q8s)) != SVS_OK)
    return rc;
  return c->q8f.grow(s.q8f);
}

// Shared passes (pass_share.h): search pipe->seq, planned as p, goes into the mailbox, and the host's copy of the claim
// rule says whether its own pass gets a thin grid.  Writes p.share* and the pipeline's owner and claim count; launches nothing.
static void publish_search(const svs_index* idx, AheadPipe* pipe, const Ctx* c, SearchPlan& p, const float* q_dev, bool claimable) {
  p.share = pipe;
  p.share_num = pipe->base + pipe->seq;
  p.share_reach = pipe->base + pipe->covered + AHEAD_RING - 1;
  p.share_epoch = idx->geo_epoch.load();
  MailEntry* m = &pipe->mailbox[p.share_num & (MAILBOX_SIZE - 1)];
  __atomic_store_n(&m->tag, (uint64_t)0, __ATOMIC_RELAXED);
  __atomic_thread_fence(__ATOMIC_RELEASE);
  const uint64_t f[7] = {(uint64_t)(uintptr_t)q_dev, (uint64_t)(uintptr_t)c->scores.p, (uint64_t)(uintptr_t)half_rows_of(idx, p.route),
                         (uint64_t)idx->n, p.share_epoch, (uint64_t)idx->ld, claimable ? MAIL_CLAIMABLE : 0u};
  for (int w = 0; w < 7; ++w) __atomic_store_n(&m->tag + 1 + w, f[w], __ATOMIC_RELAXED);
  __atomic_store_n(&m->tag, p.share_num + 1, __ATOMIC_RELEASE);
  // The grid of this search's own pass.  The claim rule, restated: the search joins the run of the last search the
  // host took for an owner when it is the next number, the run is short of the limit, it is claimable and within the
  // owner's reach, and its pass reads what the owner's reads.  The owner's claim kernel will then find it -- it is
  // published -- unless that kernel has run already: the mirrored counters (plain loads, a hint) say how many have.
  AheadPipe::Owner& o = pipe->owner;
  const bool joins = o.valid && p.share_num == o.next && o.next - o.num < (uint64_t)pipe->share_limit && claimable &&
                     p.share_num <= o.reach && f[2] == o.rows && f[3] == o.n && f[4] == o.epoch && f[5] == o.ld;
  pipe->claims += 1;   // (this search's own claim kernel: enqueue_score_half launches it first)
  if (joins && (int32_t)(pipe->claims_run() - o.ordinal) < 0) {
    o.next += 1;
    p.share_thin = true;
  } else {
    o = AheadPipe::Owner{true, p.share_num, p.share_num + 1, p.share_reach, f[2], f[3], f[4], f[5], pipe->claims};
  }
  const int64_t mode = g_tune_thin.load();
  if (mode) p.share_thin = mode == 2;
}

// One single-query search through the pipeline: score half on the pass stream (behind the query's event and, once
// per group of passes, behind a selection that covers the scratch the group overwrites: AheadPipe), selection half
// on the caller's stream behind the pass.  The caller's stream waits for the event the pass's last kernel carries
// (`e1` on a timed step); a pipeline made under svs_internal_tune(4, 1) records pass_done behind every pass and
// waits in front of every pass instead.
static int enqueue_ahead(svs_index* idx, AheadPipe* pipe, const float* q_dev, int k, int count, float* out_s, int64_t* out_r,
                         hipStream_t st, hipEvent_t query_ready) {
  std::lock_guard<std::mutex> lk(pipe->mu);
  // growing scratch frees buffers that earlier searches may still read: drain first, then grow every context of
  // the ring, so that the calls that follow allocate nothing
  const int variant = idx->variant.load();
  const SingleRoute plain = single_route(idx, variant, false);   // (screening is decided by the plan, behind the waits)
  const SingleScratch need = single_scratch(idx, plain, select_path(idx->n, count));
  bool fits = true;
  for (int j = 0; j < AHEAD_RING; ++j) fits = fits && ahead_scratch_ok(pipe->ctx[j], need);
  if (!fits) {
    if (pipe->seq) HIP_TRY(pipe_drain(pipe));
    for (int j = 0; j < AHEAD_RING; ++j) {
      const int rc = ahead_scratch_grow(pipe->ctx[j], need, pipe->pass);
      if (rc != SVS_OK) return rc;
    }
  }
  const uint64_t i = pipe->seq;
  const int j = (int)(i % AHEAD_RING);
  Ctx* c = pipe->ctx[j];
  if (query_ready) HIP_TRY(hipStreamWaitEvent(pipe->pass, query_ready, 0));
  if (i >= (uint64_t)AHEAD_LAG && (pipe->per_pass || i % AHEAD_GROUP == 0)) {
    HIP_TRY(hipStreamWaitEvent(pipe->pass, pipe->sel_done[(i - AHEAD_LAG) % AHEAD_RING], 0));
    idx->ahead_waits.fetch_add(1);
    pipe->covered = i - AHEAD_LAG + 1;
  }
  SearchPlan p;
  int rc = plan_search(idx, c, 1, k, count, pipe->pass, false, variant, &p);
  if (rc == SVS_OK && p.route.query != plain.query) rc = fail(SVS_ERR_INVALID, "internal: the ring's scratch was sized for another query staging");
  // Published before anything of this call is launched; not a query pad_query would copy (the copy lives in the context,
  // which the next search of the ring slot overwrites).  Claimable by an earlier pass: the query is complete now (no
  // event of its own), and no timed step (its events must bracket a pass that did its work).
  if (rc == SVS_OK && pipe->share_limit > 1 && !pipe->per_pass && p.path_a && p.route.shares && !query_needs_copy(idx, q_dev))
    publish_search(idx, pipe, c, p, q_dev, !query_ready && !p.timed);
  else
    pipe->owner.valid = false;   // (a search that publishes nothing ends every run)
  if (rc == SVS_OK && p.timed) idx->ahead_records.fetch_add(1);   // (e0: a start event of the extended launch is a marker of its own, so it stays a record)
  hipEvent_t done = rc == SVS_OK && p.timed && !pipe->per_pass ? p.ev.e1 : pipe->pass_done[j];
  if (!pipe->per_pass) p.pass_stop = done;
  if (rc == SVS_OK) rc = enqueue_score_half(idx, c, p, q_dev, pipe->pass);
  auto hip_step = [&](hipError_t e, const char* what) {
    if (rc == SVS_OK && e != hipSuccess) rc = fail(SVS_ERR_DEVICE, "run-ahead pipeline, %s: %s", what, hipGetErrorString(e));
  };
  if (rc == SVS_OK) {
    if (p.pass_bound) idx->ahead_bound.fetch_add(1);
    else if (p.timed) idx->ahead_records.fetch_add(1);           // (e1, recorded by the score half)
    if (!p.pass_bound && done != p.ev.e1) {
      hip_step(hipEventRecord(done, pipe->pass), "pass event");
      idx->ahead_records.fetch_add(1);
    }
  }
  if (rc == SVS_OK) hip_step(hipStreamWaitEvent(st, done, 0), "wait for the pass");
  if (rc == SVS_OK) rc = enqueue_select_half(idx, c, p, out_s, out_r, st);
  if (rc == SVS_OK) hip_step(hipEventRecord(pipe->sel_done[j], st), "selection event");
  if (rc != SVS_OK) {   // nothing half enqueued outlives a failed call (the drain also starts the ring over)
    (void)hipStreamSynchronize(st);
    (void)pipe_drain(pipe);
    pipe->base += 1;    // (a pass may have served the search this call published: its number is not used again)
    return rc;
  }
  pipe->used[j] = true;
  pipe->seq++;
  return SVS_OK;
}

// svs_index_search_device and svs_index_search_device_ahead (ahead: single queries go through the caller stream's
// pipeline; everything else is the plain call, behind the query's event if one was given)
static int32_t search_device(svs_index* idx, const float* dev_queries, int32_t nq, int32_t d, int32_t k, float* dev_out_scores,
                             int64_t* dev_out_rows, int32_t* out_count, void* hip_stream, bool ahead, void* query_ready_event) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_query_args(idx, dev_queries, nq, d);
  if (rc != SVS_OK) return rc;
  const int count = (int)std::min<int64_t>(std::max(k, 0), idx->n - (int64_t)idx->dead_list.size());
  if (out_count) *out_count = count;
  if (nq == 0 || k <= 0) return SVS_OK;
  if (!dev_out_scores || !dev_out_rows) return fail(SVS_ERR_INVALID, "null output");
  HIP_TRY(hipSetDevice(idx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (ahead && nq == 1) {
    AheadPipe* pipe = nullptr;
    if ((rc = pipe_get(idx, st, &pipe)) != SVS_OK) return rc;
    if (pipe) {
      idx->ahead_calls.fetch_add(1);
      return enqueue_ahead(idx, pipe, dev_queries, k, count, dev_out_scores, dev_out_rows, st, (hipEvent_t)query_ready_event);
    }
    idx->ahead_plain.fetch_add(1);
  }
  if (ahead && query_ready_event) HIP_TRY(hipStreamWaitEvent(st, (hipEvent_t)query_ready_event, 0));
  Ctx* c = nullptr;
  if ((rc = ctx_acquire(idx, st, false, &c)) != SVS_OK) return rc;
  CtxGuard cg{idx, c};
  // growing scratch frees buffers that earlier work on this stream may still read
  const size_t need_scores = (size_t)nq * (size_t)score_stride(idx->n);
  if (c->async_pending && (need_scores > c->scores.cap || (size_t)nq > c->hist_cap)) HIP_TRY(hipStreamSynchronize(st));
  rc = enqueue_search(idx, c, dev_queries, nq, k, count, dev_out_scores, dev_out_rows, st);
  c->last_stream = st;
  c->async_pending = true;
  return rc;
}

int32_t svs_index_search_device(svs_index* idx, const float* dev_queries, int32_t nq, int32_t d,
                                int32_t k, float* dev_out_scores, int64_t* dev_out_rows,
                                int32_t* out_count, void* hip_stream) {
  return search_device(idx, dev_queries, nq, d, k, dev_out_scores, dev_out_rows, out_count, hip_stream, false, nullptr);
}

int32_t svs_index_search_device_ahead(svs_index* idx, const float* dev_query, int32_t nq, int32_t d, int32_t k,
                                      float* dev_out_scores, int64_t* dev_out_rows, int32_t* out_count,
                                      void* hip_stream, void* query_ready_event) {
  return search_device(idx, dev_query, nq, d, k, dev_out_scores, dev_out_rows, out_count, hip_stream, true, query_ready_event);
}

int32_t svs_index_scores_n(svs_index* idx, const float* query, int32_t d, float* out_scores, int64_t out_capacity,
                           int64_t* out_n) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (appends / commits take it exclusively: idx->n cannot move below)
  if (out_n) *out_n = idx->n;
  int rc = check_query_args(idx, query, 1, d);
  if (rc != SVS_OK) return rc;
  if (!out_scores) return fail(SVS_ERR_INVALID, "null output");
  if (out_capacity < idx->n)
    return fail(SVS_ERR_INVALID, "svs_index_scores_n: the index holds %lld rows, the output buffer %lld floats "
                                 "(rows were appended since it was sized?)", (long long)idx->n, (long long)out_capacity);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  if ((rc = c->q_dev.grow((size_t)d)) != SVS_OK) return rc;
  if ((rc = c->scores.grow((size_t)score_stride(idx->n))) != SVS_OK) return rc;
  const hipStream_t st = fr.stream();
  HIP_TRY(hipMemcpyAsync(c->q_dev, query, (size_t)d * sizeof(float), hipMemcpyHostToDevice, st));
  if ((rc = launch_query_scores(idx, c, single_route(idx, idx->variant.load(), false), 0, st)) != SVS_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_scores, c->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, st));
  return fr.wait();
}

int32_t svs_index_search_rows(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                              const int64_t* rows, int64_t nrows, float* out_scores, int64_t* out_rows,
                              int32_t* out_count) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (out_count) *out_count = 0;
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  const int64_t lo = idx->row_offset;
  bool ascending;
  if ((rc = check_row_list(rows, nrows, lo, idx->n, &ascending)) != SVS_OK) return rc;
  if (nq == 0 || nrows == 0 || k <= 0) return SVS_OK;
  if (!out_scores || !out_rows) return fail(SVS_ERR_INVALID, "null output");
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  // S = the live listed rows, ascending, as local u32 rows in pinned memory (the upload's source)
  if ((rc = c->list_pin.grow((size_t)nrows)) != SVS_OK) return rc;
  uint32_t* S = c->list_pin;
  int64_t m = 0;
  try {
    std::vector<uint32_t> tmp;
    m = live_rows_ascending(rows, nrows, lo, idx->dead_flag.data(), ascending, tmp, S);
  } catch (const std::bad_alloc&) {
    return fail(SVS_ERR_NOMEM, "out of host memory for a %lld-row list", (long long)nrows);
  }
  const int count = (int)std::min<int64_t>(k, m);
  if (out_count) *out_count = count;
  if (count == 0) return SVS_OK;
  const size_t qn = (size_t)nq * (size_t)d, on = (size_t)nq * (size_t)count;
  if ((rc = c->list_dev.grow((size_t)m)) != SVS_OK) return rc;
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  const hipStream_t st = fr.stream();
  if ((rc = upload_queries(c, queries, qn, st)) != SVS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->list_dev, S, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if ((rc = search_list_chunked(idx, c, nq, d, c->list_dev, m, count, c->out_s_pin, c->out_r_pin, st)) != SVS_OK) return rc;
  if ((rc = fr.close("search_rows")) != SVS_OK) return rc;
  if ((rc = list_positions_to_rows(c->out_r_pin, on, S, m, lo, -1)) != SVS_OK) return rc;
  deliver_results(c, nq, count, k, out_scores, out_rows);
  return SVS_OK;
}

// The first write of a column (under the exclusive geometry lock): a zero column for the row CAPACITY
static int column_ensure(svs_index* idx, int column, const char* entry) {
  if (idx->cols[column]) return SVS_OK;
  const size_t bytes = label_column_bytes(std::max(idx->cap, idx->n));
  uint32_t* col = nullptr;
  HIP_TRY(hipMalloc((void**)&col, bytes));
  const hipError_t e = hipMemset(col, 0, bytes);
  if (e != hipSuccess) {
    (void)hipFree(col);
    return fail(SVS_ERR_DEVICE, "%s: %s", entry, hipGetErrorString(e));
  }
  idx->cols[column] = col;
  idx->col_bytes[column] = bytes;
  return SVS_OK;
}

static int check_column(const char* entry, int32_t column) {
  return column >= 0 && column < SVS_COLUMNS_MAX ? (int)SVS_OK
      : fail(SVS_ERR_INVALID, "%s: column %d; an index has columns 0 .. %d", entry, (int)column, SVS_COLUMNS_MAX - 1);
}

// svs_index_set_labels (column 0) and svs_index_set_column
static int32_t column_set(svs_index* idx, const char* entry, int column, int64_t row0, int64_t nrows, const uint32_t* labels) {
  RefGuard guard(idx);
  std::unique_lock<std::shared_mutex> geo(idx->rw);   // no filtered search is between its count and its write
  if (nrows == 0) return SVS_OK;
  int64_t r0;
  int rc = label_range(idx, entry, row0, nrows, &r0);
  if (rc != SVS_OK) return rc;
  if (!labels) return fail(SVS_ERR_INVALID, column ? "null values" : "null labels");
  HIP_TRY(hipSetDevice(idx->device));
  if ((rc = column_ensure(idx, column, entry)) != SVS_OK) return rc;
  // (svs_index_search_labeled, svs_index_search_by_label and svs_index_get_labels read the column, blocking and under the
  //  shared lock; svs_index_assign with vector_labels is the one other writer, blocking and under the exclusive lock like
  //  this call; reserve, append and compact carry the column along under the exclusive lock too: nothing enqueued can be
  //  reading or writing it now)
  HIP_TRY(hipMemcpy(idx->cols[column] + r0, labels, (size_t)nrows * sizeof(uint32_t), hipMemcpyHostToDevice));
  return SVS_OK;
}

// svs_index_get_labels (column 0) and svs_index_get_column
static int32_t column_get(svs_index* idx, const char* entry, int column, int64_t row0, int64_t nrows, uint32_t* out) {
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  if (nrows == 0) return SVS_OK;
  int64_t r0;
  const int rc = label_range(idx, entry, row0, nrows, &r0);
  if (rc != SVS_OK) return rc;
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  if (!idx->cols[column]) {
    memset(out, 0, (size_t)nrows * sizeof(uint32_t));
    return SVS_OK;
  }
  HIP_TRY(hipSetDevice(idx->device));
  HIP_TRY(hipMemcpy(out, idx->cols[column] + r0, (size_t)nrows * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return SVS_OK;
}

int32_t svs_index_set_labels(svs_index* idx, int64_t row0, int64_t nrows, const uint32_t* labels) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  return column_set(idx, "svs_index_set_labels", 0, row0, nrows, labels);
}

int32_t svs_index_get_labels(svs_index* idx, int64_t row0, int64_t nrows, uint32_t* out) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  return column_get(idx, "svs_index_get_labels", 0, row0, nrows, out);
}

int32_t svs_index_set_column(svs_index* idx, int32_t column, int64_t row0, int64_t nrows, const uint32_t* values) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  const int rc = check_column("svs_index_set_column", column);
  return rc != SVS_OK ? rc : column_set(idx, "svs_index_set_column", column, row0, nrows, values);
}

int32_t svs_index_get_column(svs_index* idx, int32_t column, int64_t row0, int64_t nrows, uint32_t* out) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  const int rc = check_column("svs_index_get_column", column);
  return rc != SVS_OK ? rc : column_get(idx, "svs_index_get_column", column, row0, nrows, out);
}

int32_t svs_internal_labels_strip(void) { return LB_STRIP; }

int32_t svs_index_search_labeled(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, const uint32_t* labels,
                                 int32_t nlabels, float* out_scores, int64_t* out_rows, int32_t* out_count, int64_t* out_matched) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_labels, mask_rows, compact take it exclusively: the count and the write see one column)
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  LabelSet ls;
  if ((rc = LabelSet::check(labels, nlabels)) != SVS_OK || (rc = ls.build("svs_index_search_labeled", labels, nlabels)) != SVS_OK) return rc;
  const int nset = ls.nset;
  const bool ranks = nq > 0 && k > 0 && nset > 0;   // results are wanted, if a row matches
  if (ranks && (!out_scores || !out_rows)) return fail(SVS_ERR_INVALID, "null output");
  if (ranks && (rc = check_gather_rows(idx, "svs_index_search_labeled")) != SVS_OK) return rc;
  if (nset == 0) return filtered_done(out_count, out_matched, 0, 0);   // the empty set: no row
  return filtered_search(idx, ls, FilteredNames{"search_labeled", "label_count_kernel", "label_write_kernel"}, nset, ranks, queries, nq, d, k,
                         out_scores, out_rows, out_count, out_matched);
}

// ---- svs_index_search_where (where.h)
static_assert(SVS_COLUMNS_MAX == WH_COLS && SVS_WHERE_MAX_TERMS == WH_MAX_TERMS, "where.h's kernels are built for the header's limits");
static_assert(SVS_WHERE_IN == WH_IN && SVS_WHERE_RANGE == WH_RANGE && SVS_WHERE_ANY_BITS == WH_ANY_BITS && SVS_WHERE_ALL_BITS == WH_ALL_BITS,
              "where.h's kernels take the header's op codes");

// A caller's terms, checked, and their kernel form: every IN term's set sorted and without repeats; the sets of two
// members or more one after another in `image` (at most SVS_LABELS_MAX_SET words: the kernels' LDS image).  entry: the
// ABI name the messages begin with.
struct WherePlan {
  using Filter = WhereFilter;
  WhereTerm t[WH_MAX_TERMS] = {};
  int nterms = 0;
  uint32_t col_mask = 0;
  std::vector<uint32_t> image;
  int build(const svs_where_term_t* terms, int32_t nterms_in, const char* entry = "svs_index_search_where") {
    if (nterms_in < 0) return fail(SVS_ERR_INVALID, "nterms must be >= 0");
    if (nterms_in > SVS_WHERE_MAX_TERMS)
      return fail(SVS_ERR_UNSUPPORTED, "%s: %d terms; a predicate holds at most %d", entry, (int)nterms_in, SVS_WHERE_MAX_TERMS);
    if (nterms_in > 0 && !terms) return fail(SVS_ERR_INVALID, "null terms");
    for (int i = 0; i < nterms_in; ++i) {
      const svs_where_term_t& u = terms[i];
      int rc = check_column(entry, u.column);
      if (rc != SVS_OK) return rc;
      if (u.op < SVS_WHERE_IN || u.op > SVS_WHERE_ALL_BITS) return fail(SVS_ERR_INVALID, "%s: term %d has the unknown op %d", entry, i, (int)u.op);
      if (u.negate != 0 && u.negate != 1) return fail(SVS_ERR_INVALID, "%s: term %d: negate must be 0 or 1", entry, i);
      if (u.op == SVS_WHERE_IN && (rc = LabelSet::check(u.set, u.nset)) != SVS_OK) return rc;
    }
    size_t members = 0;
    for (int i = 0; i < nterms_in; ++i) {
      const svs_where_term_t& u = terms[i];
      WhereTerm& w = t[i];
      w = WhereTerm{u.a, u.b, 0, 0, WhereTerm::pack(u.column, u.op, u.negate)};
      col_mask |= 1u << u.column;
      if (u.op != SVS_WHERE_IN) continue;
      w.a = w.b = 0;
      std::vector<uint32_t> set;
      try {
        LabelSet::sort_distinct(set, u.set, u.nset);
        members += set.size();
        if (set.size() >= 2 && members <= (size_t)SVS_LABELS_MAX_SET) {
          w.set0 = (int32_t)image.size();
          image.insert(image.end(), set.begin(), set.end());
        }
      } catch (const std::bad_alloc&) {
        return fail(SVS_ERR_NOMEM, "out of host memory for a set of %d", (int)u.nset);
      }
      w.nset = (int32_t)set.size();
      if (set.size() == 1) w.a = set[0];
    }
    if (members > (size_t)SVS_LABELS_MAX_SET)
      return fail(SVS_ERR_UNSUPPORTED, "%s: %zu distinct set members over the IN terms; a call holds at most %d", entry, members,
                  SVS_LABELS_MAX_SET);
    nterms = nterms_in;
    return SVS_OK;
  }
  // The image goes up on st through the context's pinned copy; *f = the index's filter
  int stage(const svs_index* idx, Ctx* c, hipStream_t st, WhereFilter* f) const {
    const size_t words = image.size();
    if (words) {
      int rc;
      if ((rc = c->lab_set_pin.grow(words)) != SVS_OK || (rc = c->lab_set_dev.grow(words)) != SVS_OK) return rc;
      memcpy(c->lab_set_pin, image.data(), words * sizeof(uint32_t));
      HIP_TRY(hipMemcpyAsync(c->lab_set_dev, c->lab_set_pin, words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    *f = WhereFilter{};
    f->col0 = idx->cols[0], f->col1 = idx->cols[1], f->col2 = idx->cols[2], f->col3 = idx->cols[3];
    f->n = idx->n;
    f->dead_bits = dead_bits_of(idx);
    f->set = words ? c->lab_set_dev.p : nullptr;
    f->set_words = (int32_t)words;
    f->nterms = nterms;
    f->col_mask = col_mask;
    f->t0 = t[0], f->t1 = t[1], f->t2 = t[2], f->t3 = t[3];
    return SVS_OK;
  }
};

int32_t svs_index_search_where(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, const svs_where_term_t* terms,
                               int32_t nterms, float* out_scores, int64_t* out_rows, int32_t* out_count, int64_t* out_matched) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_column, mask_rows, compact take it exclusively: the count and the write see the same columns)
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  WherePlan plan;
  if ((rc = plan.build(terms, nterms)) != SVS_OK) return rc;
  const bool ranks = nq > 0 && k > 0;   // results are wanted, if a row matches
  if (ranks && (!out_scores || !out_rows)) return fail(SVS_ERR_INVALID, "null output");
  if (ranks && (rc = check_gather_rows(idx, "svs_index_search_where")) != SVS_OK) return rc;
  return filtered_search(idx, plan, FilteredNames{"search_where", "where_count_kernel", "where_write_kernel"}, plan.nterms, ranks, queries, nq, d,
                         k, out_scores, out_rows, out_count, out_matched);
}

int32_t svs_index_search_above(svs_index* idx, const float* queries, int32_t nq, int32_t d, const float* min_scores, int32_t limit,
                               float* out_scores, int64_t* out_rows, int32_t* out_counts, int64_t* out_totals) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  if (nq > 0 && !min_scores) return fail(SVS_ERR_INVALID, "null min_scores");
  if ((rc = check_cutoffs("svs_index_search_above", min_scores, nq)) != SVS_OK) return rc;
  if (!out_counts) return fail(SVS_ERR_INVALID, "null out_counts");
  if (limit > 0 && nq > 0 && (!out_scores || !out_rows)) return fail(SVS_ERR_INVALID, "null output");
  if (nq == 0) return SVS_OK;
  const int64_t n = idx->n;
  const int64_t live = n - (int64_t)idx->dead_list.size();
  const int lim = (int)std::min<int64_t>(std::max(limit, 0), live);   // entries a query can have
  const int ls = std::min(lim, SORT_CAP);                              // ... and the most the device writes for one
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  hipStream_t st = fr.stream();
  const size_t qn = (size_t)nq * (size_t)d, on = std::max<size_t>((size_t)nq * (size_t)ls, 1);
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  if ((rc = c->above_cnt_pin.grow((size_t)nq)) != SVS_OK || (rc = c->above_tot_pin.grow((size_t)nq)) != SVS_OK) return rc;
  if ((rc = c->scores.grow((size_t)score_stride(n))) != SVS_OK) return rc;
  if ((rc = grow_select_scratch(c, 1, st)) != SVS_OK) return rc;
  const SingleRoute route = single_route(idx, idx->variant.load(), false);   // the kernel svs_index_scores_n runs
  const uint32_t* dead_bits = dead_bits_of(idx);
  const int64_t per_block = (int64_t)FA_THREADS * SEL_VPT * 4;
  const unsigned blocks = (unsigned)((n + per_block - 1) / per_block);
  if ((rc = upload_queries(c, queries, qn, st)) != SVS_OK) return rc;
  // every query back to back: score pass, filter, final -- the context's one score vector, header and candidate list
  // are reused in stream order; no host wait in between
  for (int32_t q = 0; q < nq; ++q) {
    if ((rc = launch_query_scores(idx, c, route, q, st)) != SVS_OK) return rc;
    launch_record("above_filter_kernel", n, 1);
    hipLaunchKernelGGL(above_filter_kernel, dim3(blocks), dim3(FA_THREADS), 0, st, (const float*)c->scores.p, n, score_key(min_scores[q]),
                       dead_bits, c->hist.p, c->cand.p);
    hipLaunchKernelGGL(above_final_kernel, dim3(1), dim3(FINAL_THREADS), 0, st, c->hist.p, (const uint64_t*)c->cand.p, lim, idx->row_offset,
                       c->out_s_pin + (size_t)q * ls, c->out_r_pin + (size_t)q * ls, c->above_cnt_pin + q, c->above_tot_pin + q);
  }
  if ((rc = fr.close("search_above")) != SVS_OK) return rc;
  deliver_strided(out_scores, limit, c->out_s_pin.p, ls, nq, c->above_cnt_pin.p);   // (the device-complete queries)
  deliver_strided(out_rows, limit, c->out_r_pin.p, ls, nq, c->above_cnt_pin.p);
  for (int32_t q = 0; q < nq; ++q) {
    const int64_t total = c->above_tot_pin[q];
    int count = c->above_cnt_pin[q];
    if (count < 0) {
      // Outside the device-complete zone (the list overflowed, or the wanted prefix is longer than the LDS sort): the
      // exact top-k stage over the same score vector, masked, with k = min(limit, total) -- the best that many live
      // rows are the first that many rows at or above the cut-off.
      count = (int)std::min<int64_t>(lim, total);
      if ((rc = c->redo_s_pin.grow((size_t)count)) != SVS_OK || (rc = c->redo_r_pin.grow((size_t)count)) != SVS_OK) return rc;
      st = fr.stream();
      if ((rc = launch_query_scores(idx, c, route, q, st)) != SVS_OK) return rc;
      const SelectPath path = select_path(n, count);   // (recorded: which stage the re-run took)
      launch_record(path == SelectPath::WINDOW ? "select_window_hist_kernel" : (path == SelectPath::SORT ? "keys_build_kernel" : "select_final_kernel"), n, 1);
      if ((rc = select_live(idx, c, count, c->redo_s_pin, c->redo_r_pin, st)) != SVS_OK) return rc;
      if ((rc = fr.close("search_above", true)) != SVS_OK) return rc;
      memcpy(out_scores + (size_t)q * limit, c->redo_s_pin, (size_t)count * sizeof(float));
      memcpy(out_rows + (size_t)q * limit, c->redo_r_pin, (size_t)count * sizeof(int64_t));
    }
    out_counts[q] = count;
    if (out_totals) out_totals[q] = total;
  }
  return SVS_OK;
}

int32_t svs_index_search_combined(svs_index* idx, const float* vectors, int32_t nq, int32_t m, int32_t d, const float* weights, int32_t op,
                                  int32_t k, float* out_scores, int64_t* out_rows, int32_t* out_count) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "svs_index_search_combined: null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_combined_args("svs_index_search_combined", idx, vectors, nq, m, d, weights, op);
  if (rc != SVS_OK) return rc;
  if (k < 0) return fail(SVS_ERR_INVALID, "svs_index_search_combined: k must be >= 0");
  const int64_t n = idx->n;
  const int count = (int)std::min<int64_t>(k, n - (int64_t)idx->dead_list.size());
  if (nq > 0 && count > 0 && (!out_scores || !out_rows)) return fail(SVS_ERR_INVALID, "svs_index_search_combined: null output");
  if (out_count) *out_count = count;
  if (nq == 0 || count == 0) return SVS_OK;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  const CombineRoute route = combine_route(idx, idx->variant.load(), m, (int)g_tune_combine_route.load());
  const int64_t sstride = score_stride(n);
  const size_t vn = (size_t)nq * m * d, wn = (size_t)nq * m, on = (size_t)nq * (size_t)count;
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  if ((rc = c->scores.grow((size_t)(route.fused ? 1 : m) * sstride)) != SVS_OK) return rc;
  if (select_path(n, count) == SelectPath::WINDOW && (rc = grow_select_scratch(c, 1, st)) != SVS_OK) return rc;
  if ((rc = upload_combined(c, vectors, weights, vn, wn, st)) != SVS_OK) return rc;
  // every combined query back to back: score pass(es), tombstone mask, selection -- the context's score vectors and
  // selection scratch are reused in stream order; no host wait in between
  for (int32_t q = 0; q < nq; ++q) {
    const ScoreSink fold{true, c->q_dev + vn + (size_t)q * m, op};
    if ((rc = enqueue_vector_scores(idx, c, route, c->q_dev + (size_t)q * m * d, m, sstride, fold, st)) != SVS_OK) return rc;
    if ((rc = select_live(idx, c, count, c->out_s_pin + (size_t)q * count, c->out_r_pin + (size_t)q * count, st)) != SVS_OK) return rc;
  }
  if ((rc = fr.close("search_combined")) != SVS_OK) return rc;
  deliver_results(c, nq, count, k, out_scores, out_rows);
  return SVS_OK;
}

// The two test hooks of the vector pass: one combined query on a forced route, timed (svs_internal_score_pass_ms), its
// scores copied out -- folded under (weights, op): out[0 .. n); stored: vector j's at out[j * n ..).
static int32_t internal_vector_scores(const char* entry, bool fold, svs_index* idx, const float* vectors, int32_t m, int32_t d, const float* weights,
                                      int32_t op, int32_t route, float* out, int64_t capacity) {
  launch_reset();
  g_score_pass_ms = -1.0;
  if (!idx) return fail(SVS_ERR_INVALID, "%s: null index", entry);
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  int rc = check_combined_args(entry, idx, vectors, 1, m, d, weights, op);
  if (rc != SVS_OK) return rc;
  if (route < 0 || route > 2) return fail(SVS_ERR_INVALID, "%s: route %d", entry, (int)route);
  const int64_t n = idx->n;
  const int vectors_out = fold ? 1 : m;
  if (!out || capacity < vectors_out * n)
    return fail(SVS_ERR_INVALID, "%s: %d score vectors over %lld rows, the output holds %lld floats", entry, vectors_out, (long long)n, (long long)capacity);
  if (n == 0) return SVS_OK;
  const CombineRoute r = combine_route(idx, idx->variant.load(), m, route);
  if (route == 1 && !r.has_fused) return fail(SVS_ERR_UNSUPPORTED, "%s: rows of %d elements have no fused kernel", entry, idx->ld);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  const int64_t sstride = score_stride(n);
  const size_t vn = (size_t)m * d;
  if ((rc = c->scores.grow((size_t)(fold && r.fused ? 1 : m) * sstride)) != SVS_OK) return rc;
  if ((rc = upload_combined(c, vectors, weights, vn, (size_t)m, st)) != SVS_OK) return rc;
  const TimedSpan t_pass(idx->timing.load() > 0);
  t_pass.begin(st);
  if ((rc = enqueue_vector_scores(idx, c, r, c->q_dev, m, sstride, fold ? ScoreSink{true, c->q_dev + vn, op} : kStoreScores, st)) != SVS_OK) return rc;
  t_pass.end(st);
  if ((rc = fr.launched(entry + sizeof("svs_internal_") - 1)) != SVS_OK) return rc;   // ("combined_scores launch: ...")
  if (fold)
    HIP_TRY(hipMemcpyAsync(out, c->scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, st));
  else
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)n * sizeof(float), c->scores, (size_t)sstride * sizeof(float), (size_t)n * sizeof(float), (size_t)m,
                             hipMemcpyDeviceToHost, st));
  if ((rc = fr.wait()) != SVS_OK) return rc;
  g_score_pass_ms = t_pass.ms();
  return SVS_OK;
}

int32_t svs_internal_combined_scores(svs_index* idx, const float* vectors, int32_t m, int32_t d, const float* weights, int32_t op, int32_t route,
                                     float* out, int64_t capacity) {
  return internal_vector_scores("svs_internal_combined_scores", true, idx, vectors, m, d, weights, op, route, out, capacity);
}

int32_t svs_internal_multi_scores(svs_index* idx, const float* vectors, int32_t m, int32_t d, int32_t route, float* out, int64_t capacity) {
  return internal_vector_scores("svs_internal_multi_scores", false, idx, vectors, m, d, nullptr, SVS_COMBINE_MAX, route, out, capacity);
}

int32_t svs_internal_by_label_geometry(int32_t* out) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  out[0] = BL_STRIP;
  out[1] = BL_GRID_MAX;
  return SVS_OK;
}

int32_t svs_index_search_by_label(svs_index* idx, const float* queries, int32_t nq, int32_t d, const uint32_t* labels, int32_t nlabels,
                                  const float* min_scores, int32_t k, uint32_t* out_labels, float* out_scores, int64_t* out_rows,
                                  int64_t* out_totals, int32_t* out_counts, int32_t* out_groups) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_labels, mask_rows, compact take it exclusively: every query sees one column)
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  if ((rc = LabelSet::check(labels, nlabels)) != SVS_OK) return rc;
  if ((rc = check_cutoffs("svs_index_search_by_label", min_scores, nq)) != SVS_OK) return rc;
  if (!out_counts) return fail(SVS_ERR_INVALID, "null out_counts");
  LabelSet ls;
  if ((rc = ls.build("svs_index_search_by_label", labels, nlabels)) != SVS_OK) return rc;
  const int nset = ls.nset;
  if (k > 0 && nq > 0 && nset > 0 && (!out_labels || !out_scores || !out_rows || !out_totals)) return fail(SVS_ERR_INVALID, "null output");
  if (nq == 0 || nset == 0) {
    for (int32_t q = 0; q < nq; ++q) {
      out_counts[q] = 0;
      if (out_groups) out_groups[q] = 0;
    }
    return SVS_OK;
  }
  const int64_t n = idx->n;
  const int ks = std::min(std::max(k, 0), nset);   // entries a query can have
  const int cross = (int)g_tune_by_label_cross.load();
  const unsigned blocks = (unsigned)std::min<int64_t>((n + BL_STRIP - 1) / BL_STRIP, BL_GRID_MAX);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  hipStream_t st = fr.stream();
  const size_t qn = (size_t)nq * (size_t)d, on = std::max<size_t>((size_t)nq * (size_t)ks, 1);
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  if ((rc = c->bl_lab_pin.grow(on)) != SVS_OK || (rc = c->bl_tot_pin.grow(on)) != SVS_OK || (rc = c->bl_cnt_pin.grow((size_t)nq * 2)) != SVS_OK) return rc;
  if ((rc = c->scores.grow((size_t)score_stride(n))) != SVS_OK) return rc;
  if (cross == BL_PARTIALS) {
    if ((rc = c->bl_part_best.grow((size_t)blocks * nset)) != SVS_OK || (rc = c->bl_part_cnt.grow((size_t)blocks * nset)) != SVS_OK) return rc;
  } else if (!c->bl_tab.p) {
    if ((rc = c->bl_tab.grow(BL_TAB_WORDS)) != SVS_OK) return rc;
    // zeroed once; by_label_final_kernel leaves it zeroed after every query
    HIP_TRY(hipMemsetAsync(c->bl_tab, 0, (size_t)BL_TAB_WORDS * sizeof(unsigned long long), st));
  }
  const SingleRoute route = single_route(idx, idx->variant.load(), false);   // the kernel svs_index_scores_n runs
  if ((rc = upload_queries(c, queries, qn, st)) != SVS_OK) return rc;
  LabelFilter f;
  if ((rc = ls.stage(idx, c, st, &f)) != SVS_OK) return rc;
  // every query back to back: score pass, reduce, final -- the context's one score vector and one table are reused in
  // stream order; no host wait in between
  for (int32_t q = 0; q < nq; ++q) {
    const uint32_t tkey = score_key(min_scores ? min_scores[q] : -std::numeric_limits<float>::infinity());
    if ((rc = launch_query_scores(idx, c, route, q, st)) != SVS_OK) return rc;
    launch_record("by_label_reduce_kernel", n, 1);
    if (cross == BL_PARTIALS)
      hipLaunchKernelGGL(by_label_reduce_kernel<BL_PARTIALS>, dim3(blocks), dim3(BL_THREADS), 0, st, f, (const float*)c->scores.p, tkey,
                         (unsigned long long*)nullptr, c->bl_part_best.p, c->bl_part_cnt.p);
    else
      hipLaunchKernelGGL(by_label_reduce_kernel<BL_ATOMIC>, dim3(blocks), dim3(BL_THREADS), 0, st, f, (const float*)c->scores.p, tkey,
                         c->bl_tab.p, (unsigned long long*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(by_label_final_kernel, dim3(1), dim3(BL_FINAL_THREADS), 0, st, c->bl_tab.p, (const unsigned long long*)c->bl_part_best.p,
                       (const uint32_t*)c->bl_part_cnt.p, cross == BL_PARTIALS ? (int)blocks : 0, (const uint32_t*)c->lab_set_dev.p, f.single, nset,
                       k, idx->row_offset, c->bl_lab_pin + (size_t)q * ks, c->out_s_pin + (size_t)q * ks, c->out_r_pin + (size_t)q * ks,
                       c->bl_tot_pin + (size_t)q * ks, c->bl_cnt_pin + q, c->bl_cnt_pin + nq + q);
  }
  if ((rc = fr.close("search_by_label")) != SVS_OK) return rc;
  for (int32_t q = 0; q < nq; ++q) {
    const int count = c->bl_cnt_pin[q], groups = c->bl_cnt_pin[nq + q];
    if (count < 0 || count > ks || groups < count || groups > nset)
      return fail(SVS_ERR_DEVICE, "search_by_label: query %d came back with %d entries of %d groups (%d labels)", (int)q, count, groups, nset);
  }
  deliver_strided(out_labels, k, c->bl_lab_pin.p, ks, nq, c->bl_cnt_pin.p);
  deliver_strided(out_scores, k, c->out_s_pin.p, ks, nq, c->bl_cnt_pin.p);
  deliver_strided(out_rows, k, c->out_r_pin.p, ks, nq, c->bl_cnt_pin.p);
  deliver_strided(out_totals, k, c->bl_tot_pin.p, ks, nq, c->bl_cnt_pin.p);
  memcpy(out_counts, c->bl_cnt_pin, (size_t)nq * sizeof(int32_t));
  if (out_groups) memcpy(out_groups, c->bl_cnt_pin + nq, (size_t)nq * sizeof(int32_t));
  return SVS_OK;
}

// ---- the collapse entries (collapse.h, collapse_scope.h, collapse_combine.h): what the four share --------------------
static_assert(SVS_COLLAPSE_ZERO_IS_GROUP == CL_ZERO_IS_GROUP && SVS_COLLAPSE_ZERO_SINGLE == CL_ZERO_SINGLE, "collapse.h's kernels take the header's zero modes");

// What an entry is given to write into (matched: the scoped entries'), and the one way of writing the answer when
// nothing is in scope: no row, no group
struct CollapseOut {
  float* scores;
  int64_t* rows;
  uint32_t* values;
  int32_t* counts;
  int64_t* groups;
  int64_t* matched;
};

static int32_t collapse_empty(const CollapseOut& o, int32_t nq) {
  for (int32_t q = 0; q < nq; ++q) {
    o.counts[q] = 0;
    if (o.groups) o.groups[q] = 0;
  }
  if (o.matched) *o.matched = 0;
  return SVS_OK;
}

// The checks the entries share, in one order (the caller has checked its queries or vectors)
static int check_collapse_args(const char* entry, int32_t nq, int32_t k, int32_t column, int32_t zero_mode, const CollapseOut& o) {
  const int rc = check_column(entry, column);
  if (rc != SVS_OK) return rc;
  if (zero_mode != SVS_COLLAPSE_ZERO_IS_GROUP && zero_mode != SVS_COLLAPSE_ZERO_SINGLE)
    return fail(SVS_ERR_INVALID, "%s: zero_mode %d", entry, (int)zero_mode);
  if (!o.counts) return fail(SVS_ERR_INVALID, "%s: null out_counts", entry);
  if (k > 0 && nq > 0 && (!o.scores || !o.rows || !o.values)) return fail(SVS_ERR_INVALID, "%s: null output", entry);
  return SVS_OK;
}

// What differs between the entries behind a query's score vector
struct CollapseScope {
  const char* name;            // the call in its messages
  int64_t rows;                // what a score vector covers: the index's n rows, or the positions of c->list_dev
  int64_t bound;               // no query has more groups: the live rows, or the rows in scope ...
  const char* bound_what;      // ... as a message calls them
  bool listed;                 // rows are positions in c->list_dev: selected into c->lab_pos, global rows from finish()
  int vectors;                 // 0, or a combined query's m: cc_reduce / cc_mark_kernel, m keys per slot in c->cc_keys
  const uint32_t* values;      // the group column over the rows (null: never set)
  const uint32_t* dead_bits;   // the rows' tombstones (null: none among them)
  int zero_mode;
};

// The stages behind the score pass, once for every collapse entry.  prepare() sizes the outputs, the counters and the
// selection scratch and leaves the table EMPTY; query() enqueues one query's reduce, mark, fill, top-k stage and values;
// finish() reads the counters back, validates and delivers.  The table, and the keys beside it, are EMPTY (all zero)
// between queries and between calls of ANY entry on the context: cl_clean / cc_clean are false from a query's first insert
// until the fill behind its mark kernel is enqueued, so a call that left early is repaired by the next one.  The flags
// are written here (query(), empty()) and nowhere else.
struct CollapseFrame {
  svs_index* const idx;
  Ctx* const c;
  const int32_t nq, k;
  const CollapseScope s;
  const int ks;   // entries a query can have: what the top-k stage is asked for
  const int bits;
  const size_t tab_words, key_words;
  const unsigned blocks;
  const TimedSpan t_reduce, t_mark, t_clear, t_select;   // (svs_index_set_timing: around the last query's stages)
  CollapseArgs a{};

  CollapseFrame(svs_index* i, Ctx* ctx, int32_t nq_, int32_t k_, const CollapseScope& scope)
      : idx(i), c(ctx), nq(nq_), k(k_), s(scope), ks((int)std::min<int64_t>(std::max(k_, 0), scope.bound)), bits(collapse_table_bits(scope.rows)),
        tab_words(((size_t)1 << bits) * CL_SLOT_WORDS), key_words(((size_t)1 << bits) * (size_t)scope.vectors),
        blocks((unsigned)std::min<int64_t>((scope.rows + CL_STRIP - 1) / CL_STRIP, CL_GRID_MAX)), t_reduce(i->timing.load() > 0), t_mark(t_reduce.on),
        t_clear(t_reduce.on), t_select(t_reduce.on) {}

  // `words` of the table and `keys` of the key array go to EMPTY behind what is enqueued
  int empty(size_t words, size_t keys, hipStream_t st) {
    if (words) {
      HIP_TRY(hipMemsetAsync(c->cl_tab, 0, words * sizeof(unsigned long long), st));
      c->cl_clean = true;
    }
    if (keys) {   // (the keys' layout depends on m: only an all-zero array fits every m)
      HIP_TRY(hipMemsetAsync(c->cc_keys, 0, keys * sizeof(uint32_t), st));
      c->cc_clean = true;
    }
    return SVS_OK;
  }

  int prepare(hipStream_t st) {
    int rc;
    const size_t on = std::max<size_t>((size_t)nq * (size_t)ks, 1);
    if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK || (rc = c->cl_val_pin.grow(on)) != SVS_OK) return rc;
    if (s.listed && (rc = c->lab_pos.grow(on)) != SVS_OK) return rc;
    if ((rc = c->cl_cnt.grow((size_t)nq)) != SVS_OK || (rc = c->cl_cnt_pin.grow((size_t)nq)) != SVS_OK) return rc;
    if (ks > 0 && select_path(s.rows, ks) == SelectPath::WINDOW && (rc = grow_select_scratch(c, 1, st)) != SVS_OK) return rc;
    // a fresh array, or one an earlier call left early: all of it goes to empty
    const bool fresh_tab = c->cl_tab.cap < tab_words || !c->cl_clean, fresh_keys = c->cc_keys.cap < key_words || (key_words && !c->cc_clean);
    if (fresh_tab && ((rc = c->cl_tab.grow(tab_words)) != SVS_OK || (rc = empty(c->cl_tab.cap, 0, st)) != SVS_OK)) return rc;
    if (fresh_keys && ((rc = c->cc_keys.grow(key_words)) != SVS_OK || (rc = empty(0, c->cc_keys.cap, st)) != SVS_OK)) return rc;
    HIP_TRY(hipMemsetAsync(c->cl_cnt, 0, (size_t)nq * sizeof(unsigned long long), st));
    a = CollapseArgs{s.values, s.dead_bits, c->cl_tab.p, s.rows, bits, s.zero_mode == SVS_COLLAPSE_ZERO_SINGLE ? 1 : 0};
    return SVS_OK;
  }

  // Query q's stages over its score vector sv, in stream order behind its score pass.  g: a combined query's m score
  // vectors (sv is the first; the mark kernel leaves the combined scores there); null: sv holds one query's scores.
  int query(int32_t q, float* sv, int64_t sstride, const GroupCombineArgs* g, hipStream_t st) {
    const bool last = q == nq - 1;
    const dim3 grid(blocks), wg(CL_THREADS);
    int rc;
    c->cl_clean = false;
    if (g) c->cc_clean = false;
    if (last) t_reduce.begin(st);
    launch_record(g ? "cc_reduce_kernel" : "collapse_reduce_kernel", s.rows, g ? g->m : 1);
    if (g) hipLaunchKernelGGL(cc_reduce_kernel, grid, wg, 0, st, a, *g);
    else hipLaunchKernelGGL(collapse_reduce_kernel, grid, wg, 0, st, a, (const float*)sv);
    if (last) { t_reduce.end(st); t_mark.begin(st); }
    launch_record(g ? "cc_mark_kernel" : "collapse_mark_kernel", s.rows, g ? g->m : 1);
    if (g) hipLaunchKernelGGL(cc_mark_kernel, grid, wg, 0, st, a, *g, c->cl_cnt.p + q);
    else hipLaunchKernelGGL(collapse_mark_kernel, grid, wg, 0, st, a, sv, c->cl_cnt.p + q);
    if (last) { t_mark.end(st); t_clear.begin(st); }
    if ((rc = empty(tab_words, g ? key_words : 0, st)) != SVS_OK) return rc;
    if (last) t_clear.end(st);
    if (ks == 0) return SVS_OK;
    // the best ks survivors: rows of the index, or positions in the list
    int64_t* const sel = (s.listed ? c->lab_pos.p : c->out_r_pin.p) + (size_t)q * ks;
    const int64_t base = s.listed ? 0 : idx->row_offset;
    if (last) t_select.begin(st);
    if ((rc = run_select(idx, c, sv, s.rows, sstride, 1, ks, ks, c->out_s_pin + (size_t)q * ks, sel, st, base)) != SVS_OK) return rc;
    if (last) t_select.end(st);
    hipLaunchKernelGGL(collapse_values_kernel, dim3((unsigned)std::min((ks + 255) / 256, 64)), dim3(256), 0, st, (const int64_t*)sel, ks, base, s.rows,
                       s.values, c->cl_val_pin + (size_t)q * ks);
    return SVS_OK;
  }
  double select_ms() const { return ks > 0 ? t_select.ms() : -1.0; }

  // The call's last wait and its trimmed results (a list's positions -> global rows on the device first)
  int finish(HostCall& fr, const CollapseOut& o) {
    const size_t nres = (size_t)nq * (size_t)ks;
    if (s.listed && nres)
      hipLaunchKernelGGL(label_map_rows_kernel, dim3((unsigned)std::min<size_t>((nres + 255) / 256, 1024)), dim3(256), 0, fr.stream(),
                         (const int64_t*)c->lab_pos.p, (int64_t)nres, (const uint32_t*)c->list_dev.p, s.rows, idx->row_offset, c->out_r_pin.p);
    int rc = read_back(fr, s.name, {{c->cl_cnt_pin.p, c->cl_cnt.p, (size_t)nq * sizeof(unsigned long long)}});
    if (rc != SVS_OK) return rc;
    std::vector<int32_t> counts((size_t)nq);
    for (int32_t q = 0; q < nq; ++q) {
      const unsigned long long w = c->cl_cnt_pin[q];
      if (w > (unsigned long long)s.bound)
        return fail(SVS_ERR_DEVICE, "%s: query %d came back with %llu groups of %lld %s", s.name, (int)q, w, (long long)s.bound, s.bound_what);
      counts[(size_t)q] = (int32_t)std::min<unsigned long long>((unsigned long long)ks, w);
    }
    for (size_t i = 0; s.listed && i < nres; ++i)
      if (c->out_r_pin[i] < 0)
        return fail(SVS_ERR_DEVICE, "%s: result %zu of query %zu is a position outside the %lld %s", s.name, i % (size_t)ks, i / (size_t)ks,
                    (long long)s.rows, s.bound_what);
    if (ks > 0) {
      deliver_strided(o.scores, k, c->out_s_pin.p, ks, nq, counts.data());
      deliver_strided(o.rows, k, c->out_r_pin.p, ks, nq, counts.data());
      deliver_strided(o.values, k, c->cl_val_pin.p, ks, nq, counts.data());
    }
    for (int32_t q = 0; q < nq; ++q) {
      o.counts[q] = counts[(size_t)q];
      if (o.groups) o.groups[q] = (int64_t)c->cl_cnt_pin[q];
    }
    return SVS_OK;
  }
};

// ---- svs_index_search_collapsed (collapse.h)
int32_t svs_internal_collapse_geometry(int32_t* out) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  out[0] = CL_STRIP;
  out[1] = CL_GRID_MAX;
  return SVS_OK;
}

int32_t svs_internal_collapse_kernel_ms(double* out) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  for (int i = 0; i < 4; ++i) out[i] = g_collapse_ms[i];
  return SVS_OK;
}

int32_t svs_index_search_collapsed(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, int32_t column, int32_t zero_mode,
                                   float* out_scores, int64_t* out_rows, uint32_t* out_values, int32_t* out_counts, int64_t* out_groups) {
  launch_reset();
  for (double& ms : g_collapse_ms) ms = -1.0;   // (a call that fails or records nothing leaves no earlier call's times behind)
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_column, mask_rows, compact take it exclusively: every query sees one column)
  // ---- everything is validated before anything is written, allocated or launched
  const CollapseOut o{out_scores, out_rows, out_values, out_counts, out_groups, nullptr};
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK || (rc = check_collapse_args("svs_index_search_collapsed", nq, k, column, zero_mode, o)) != SVS_OK) return rc;
  if (nq == 0) return SVS_OK;
  const int64_t n = idx->n;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  const int64_t sstride = score_stride(n);
  CollapseFrame cf(idx, c, nq, k, {"search_collapsed", n, n - (int64_t)idx->dead_list.size(), "live rows", false, 0, idx->cols[column], dead_bits_of(idx), zero_mode});
  if ((rc = c->scores.grow((size_t)sstride)) != SVS_OK || (rc = cf.prepare(st)) != SVS_OK) return rc;
  const SingleRoute route = single_route(idx, idx->variant.load(), false);   // the kernel svs_index_scores_n runs
  if ((rc = upload_queries(c, queries, (size_t)nq * (size_t)d, st)) != SVS_OK) return rc;
  // every query back to back: score pass, then the frame's stages -- the context's one score vector, one table and
  // selection scratch are reused in stream order; no host wait in between
  for (int32_t q = 0; q < nq; ++q)
    if ((rc = launch_query_scores(idx, c, route, q, st)) != SVS_OK || (rc = cf.query(q, c->scores.p, sstride, nullptr, st)) != SVS_OK) return rc;
  if ((rc = cf.finish(fr, o)) != SVS_OK) return rc;
  g_collapse_ms[0] = cf.t_reduce.ms();
  g_collapse_ms[1] = cf.t_mark.ms();
  g_collapse_ms[2] = cf.t_clear.ms();
  g_collapse_ms[3] = cf.select_ms();
  return SVS_OK;
}

// ---- svs_index_search_collapsed_where, svs_index_search_collapsed_rows (collapse_scope.h)
int32_t svs_internal_collapse_scope_kernel_ms(double* out) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  for (int i = 0; i < 6; ++i) out[i] = g_collapse_scope_ms[i];
  return SVS_OK;
}

// What the two do once c->list_dev holds S (m >= 1 local rows, ascending) and c->sc_vals the group column beside it,
// both enqueued on the frame's stream, with the queries uploaded: the gather kernel scores chunks of queries over the
// list (search_list_chunked's 2 GiB rule), and every query's compact vector goes through the frame's stages with
// positions for rows.  filter_ms: what the caller's filter took.
static int32_t collapse_over_list(svs_index* idx, HostCall& fr, const char* entry, int32_t nq, int32_t d, int32_t k, int64_t m, int32_t zero_mode,
                                  const CollapseOut& o, const TimedSpan& t_filter, double filter_ms) {
  Ctx* const c = fr.c;
  int rc;
  const int64_t sstride = score_stride(m);
  const int qc = (int)std::max<int64_t>(1, std::min<int64_t>(nq, ((int64_t)2 << 30) / (4 * sstride)));   // queries per gather launch
  const hipStream_t st = fr.stream();
  // (no bitmap: S holds live rows only)
  CollapseFrame cf(idx, c, nq, k, {entry, m, m, "rows in scope", true, 0, c->sc_vals.p, nullptr, zero_mode});
  if ((rc = c->scores.grow((size_t)qc * (size_t)sstride)) != SVS_OK || (rc = cf.prepare(st)) != SVS_OK) return rc;
  const TimedSpan t_gather(idx->timing.load() > 0);
  for (int32_t q0 = 0; q0 < nq; q0 += qc) {
    const int32_t nc = std::min<int32_t>(qc, nq - q0);
    const bool last_chunk = q0 + nc == nq;   // (svs_index_set_timing: a span around the last chunk's gather)
    if (last_chunk) t_gather.begin(st);
    if ((rc = launch_gather(idx, c, c->q_dev + (size_t)q0 * d, nc, c->list_dev, m, c->scores, sstride, st)) != SVS_OK) return rc;
    if (last_chunk) t_gather.end(st);
    for (int32_t q = q0; q < q0 + nc; ++q)
      if ((rc = cf.query(q, c->scores.p + (size_t)(q - q0) * (size_t)sstride, sstride, nullptr, st)) != SVS_OK) return rc;
  }
  if ((rc = cf.finish(fr, o)) != SVS_OK) return rc;
  if (o.matched) *o.matched = m;
  const double write_ms = t_filter.ms();
  g_collapse_scope_ms[0] = filter_ms >= 0.0 && write_ms >= 0.0 ? filter_ms + write_ms : write_ms;
  g_collapse_scope_ms[1] = t_gather.ms();
  g_collapse_scope_ms[2] = cf.t_reduce.ms();
  g_collapse_scope_ms[3] = cf.t_mark.ms();
  g_collapse_scope_ms[4] = cf.t_clear.ms();
  g_collapse_scope_ms[5] = cf.select_ms();
  return SVS_OK;
}

int32_t svs_index_search_collapsed_where(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, const svs_where_term_t* terms,
                                         int32_t nterms, int32_t column, int32_t zero_mode, float* out_scores, int64_t* out_rows,
                                         uint32_t* out_values, int32_t* out_counts, int64_t* out_groups, int64_t* out_matched) {
  static const char* const kEntry = "svs_index_search_collapsed_where";
  launch_reset();
  for (double& ms : g_collapse_scope_ms) ms = -1.0;   // (a call that fails or records nothing leaves no earlier call's times behind)
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_column, mask_rows, compact take it exclusively: the count and the write see the same columns)
  // ---- everything is validated before anything is written, allocated or launched
  const CollapseOut o{out_scores, out_rows, out_values, out_counts, out_groups, out_matched};
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK || (rc = check_collapse_args(kEntry, nq, k, column, zero_mode, o)) != SVS_OK) return rc;
  WherePlan plan;
  if ((rc = plan.build(terms, nterms, kEntry)) != SVS_OK) return rc;
  if (nq == 0) return SVS_OK;
  if ((rc = check_gather_rows(idx, kEntry)) != SVS_OK) return rc;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const int64_t n = idx->n;
  if ((rc = c->lab_cnt.grow((size_t)label_strips(n) + 2)) != SVS_OK || (rc = c->lab_tot_pin.grow(1)) != SVS_OK) return rc;
  // 1. the filter goes up, the count runs; the host needs m = |S| to size the list, the table and the score vectors
  const bool timed = idx->timing.load() > 0;
  const TimedSpan t_count(timed), t_write(timed);
  hipStream_t st = fr.stream();
  WhereFilter f;
  if ((rc = plan.stage(idx, c, st, &f)) != SVS_OK) return rc;
  t_count.begin(st);
  launch_record("where_count_kernel", n, plan.nterms);
  launch_label_count(f, c->lab_cnt, st);
  t_count.end(st);
  HIP_TRY(hipMemcpyAsync(c->lab_tot_pin, c->lab_cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  if ((rc = fr.close(kEntry)) != SVS_OK) return rc;
  const int64_t m = (int64_t)c->lab_tot_pin[0];
  if (m < 0 || m > n) return fail(SVS_ERR_DEVICE, "%s: the filter counted %lld of %lld rows", kEntry, (long long)m, (long long)n);
  if (m == 0) return collapse_empty(o, nq);
  // 2. one write pass emits the list and the group column beside it
  if ((rc = c->list_dev.grow((size_t)m)) != SVS_OK || (rc = c->sc_vals.grow((size_t)score_stride(m))) != SVS_OK) return rc;
  st = fr.stream();
  if ((rc = upload_queries(c, queries, (size_t)nq * (size_t)d, st)) != SVS_OK) return rc;
  t_write.begin(st);
  launch_record("scoped_write_kernel", n, plan.nterms);
  hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(LB_THREADS), 0, st, c->lab_cnt.p + 2, label_strips(n));
  hipLaunchKernelGGL(scoped_write_kernel, dim3((unsigned)label_strips(n)), dim3(LB_THREADS), 0, st, f, (int)column,
                     (const uint32_t*)(c->lab_cnt.p + 2), c->list_dev.p, c->sc_vals.p, m);
  t_write.end(st);
  return collapse_over_list(idx, fr, kEntry, nq, d, k, m, zero_mode, o, t_write, t_count.ms());
}

int32_t svs_index_search_collapsed_rows(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, const int64_t* rows, int64_t nrows,
                                        int32_t column, int32_t zero_mode, float* out_scores, int64_t* out_rows, uint32_t* out_values,
                                        int32_t* out_counts, int64_t* out_groups, int64_t* out_matched) {
  static const char* const kEntry = "svs_index_search_collapsed_rows";
  launch_reset();
  for (double& ms : g_collapse_scope_ms) ms = -1.0;
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_column, mask_rows, compact take it exclusively: the list and the column are one state's)
  // ---- everything is validated before anything is written, allocated or launched
  const CollapseOut o{out_scores, out_rows, out_values, out_counts, out_groups, out_matched};
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK || (rc = check_collapse_args(kEntry, nq, k, column, zero_mode, o)) != SVS_OK) return rc;
  const int64_t lo = idx->row_offset;
  bool ascending;
  if ((rc = check_row_list(rows, nrows, lo, idx->n, &ascending)) != SVS_OK) return rc;
  if (nq == 0) return SVS_OK;
  if ((rc = check_gather_rows(idx, kEntry)) != SVS_OK) return rc;
  if (nrows == 0) return collapse_empty(o, nq);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  // S = the live listed rows, ascending, as local u32 rows in pinned memory (the upload's source): svs_index_search_rows'
  if ((rc = c->list_pin.grow((size_t)nrows)) != SVS_OK) return rc;
  int64_t m = 0;
  try {
    std::vector<uint32_t> tmp;
    m = live_rows_ascending(rows, nrows, lo, idx->dead_flag.data(), ascending, tmp, c->list_pin);
  } catch (const std::bad_alloc&) {
    return fail(SVS_ERR_NOMEM, "out of host memory for a %lld-row list", (long long)nrows);
  }
  if (m == 0) return collapse_empty(o, nq);
  if ((rc = c->list_dev.grow((size_t)m)) != SVS_OK || (rc = c->sc_vals.grow((size_t)score_stride(m))) != SVS_OK) return rc;
  const TimedSpan t_filter(idx->timing.load() > 0);
  const hipStream_t st = fr.stream();
  if ((rc = upload_queries(c, queries, (size_t)nq * (size_t)d, st)) != SVS_OK) return rc;
  t_filter.begin(st);
  HIP_TRY(hipMemcpyAsync(c->list_dev, c->list_pin, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  launch_record("scoped_values_kernel", m, 1);
  hipLaunchKernelGGL(scoped_values_kernel, dim3((unsigned)std::min<int64_t>((m + 255) / 256, 1024)), dim3(256), 0, st,
                     (const uint32_t*)c->list_dev.p, m, (const uint32_t*)idx->cols[column], c->sc_vals.p);
  t_filter.end(st);
  return collapse_over_list(idx, fr, kEntry, nq, d, k, m, zero_mode, o, t_filter, -1.0);
}

// ---- svs_index_search_collapsed_combined (collapse_combine.h)
int32_t svs_internal_collapsed_combined_kernel_ms(double* out) {
  if (!out) return fail(SVS_ERR_INVALID, "null output");
  for (int i = 0; i < 5; ++i) out[i] = g_collapsed_combined_ms[i];
  return SVS_OK;
}

int32_t svs_internal_score_pass_ms(double* out) { return report_ms(out, g_score_pass_ms); }

int32_t svs_index_search_collapsed_combined(svs_index* idx, const float* vectors, int32_t nq, int32_t m, int32_t d, const float* weights, int32_t op,
                                            int32_t k, int32_t column, int32_t zero_mode, float* out_scores, int64_t* out_rows,
                                            uint32_t* out_values, int32_t* out_counts, int64_t* out_groups) {
  static const char* const kEntry = "svs_index_search_collapsed_combined";
  launch_reset();
  for (double& ms : g_collapsed_combined_ms) ms = -1.0;   // (a call that fails or records nothing leaves no earlier call's times behind)
  if (!idx) return fail(SVS_ERR_INVALID, "%s: null index", kEntry);
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (set_column, mask_rows, compact take it exclusively: every query sees one column)
  // ---- everything is validated before anything is written, allocated or launched
  const CollapseOut o{out_scores, out_rows, out_values, out_counts, out_groups, nullptr};
  int rc = check_combined_args(kEntry, idx, vectors, nq, m, d, weights, op);
  if (rc != SVS_OK || (rc = check_collapse_args(kEntry, nq, k, column, zero_mode, o)) != SVS_OK) return rc;
  if (nq == 0) return SVS_OK;
  const int64_t n = idx->n;
  if (n == 0) return collapse_empty(o, nq);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  const size_t vn = (size_t)nq * m * d, wn = (size_t)nq * m;
  const int64_t sstride = score_stride(n);
  CollapseFrame cf(idx, c, nq, k, {"search_collapsed_combined", n, n - (int64_t)idx->dead_list.size(), "live rows", false, m, idx->cols[column], dead_bits_of(idx), zero_mode});
  if ((rc = c->scores.grow((size_t)m * sstride)) != SVS_OK || (rc = cf.prepare(st)) != SVS_OK) return rc;
  const CombineRoute route = combine_route(idx, idx->variant.load(), m, (int)g_tune_combine_route.load());
  if ((rc = upload_combined(c, vectors, weights, vn, wn, st)) != SVS_OK) return rc;
  const TimedSpan t_scores(idx->timing.load() > 0);
  // every query back to back: score pass(es), then the frame's stages -- the context's score vectors, table, keys and
  // selection scratch are reused in stream order; no host wait in between
  for (int32_t q = 0; q < nq; ++q) {
    const bool last = q == nq - 1;   // (svs_index_set_timing: a span around the last query's score pass)
    const GroupCombineArgs g{c->scores.p, sstride, c->q_dev + vn + (size_t)q * m, c->cc_keys.p, m, op};
    if (last) t_scores.begin(st);
    if ((rc = enqueue_vector_scores(idx, c, route, c->q_dev + (size_t)q * m * d, m, sstride, kStoreScores, st)) != SVS_OK) return rc;
    if (last) t_scores.end(st);
    if ((rc = cf.query(q, c->scores.p, sstride, &g, st)) != SVS_OK) return rc;
  }
  if ((rc = cf.finish(fr, o)) != SVS_OK) return rc;
  g_collapsed_combined_ms[0] = t_scores.ms();
  g_collapsed_combined_ms[1] = cf.t_reduce.ms();
  g_collapsed_combined_ms[2] = cf.t_mark.ms();
  g_collapsed_combined_ms[3] = cf.t_clear.ms();
  g_collapsed_combined_ms[4] = cf.select_ms();
  return SVS_OK;
}


static_assert(SVS_ASSIGN_MAX_VECTORS == AS_MAX_VECTORS, "the assign kernel's LDS count table holds SVS_ASSIGN_MAX_VECTORS slots");
static_assert(SVS_ASSIGN_MAX_VECTORS == SVS_LABELS_MAX_SET, "every label an assignment writes can be named in one labelled call");

int32_t svs_index_assign(svs_index* idx, const float* vectors, int32_t c, int32_t d, int64_t row0, int64_t nrows,
                         const uint32_t* vector_labels, int32_t* out_best, float* out_scores, int64_t* out_counts) {
  launch_reset();
  g_assign_kernel_ms = -1.0;   // (a call that fails or records nothing leaves no earlier call's time behind)
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  // with labels to write: exclusive for the whole call, as svs_index_set_labels (no labelled search is between its count
  // and its write); without: a reader like every search
  std::shared_lock<std::shared_mutex> geo_shared(idx->rw, std::defer_lock);
  std::unique_lock<std::shared_mutex> geo_excl(idx->rw, std::defer_lock);
  if (vector_labels) geo_excl.lock();
  else geo_shared.lock();
  // ---- everything is validated before anything is written, allocated or launched
  if (d != idx->d || idx->n == 0 || idx->d == 0)
    return fail(SVS_ERR_SHAPE, "shapes (%lld,%d) and (%d,) not aligned: %d (dim 1) != %d (dim 0)", (long long)idx->n, idx->d, d, idx->d, d);
  if (c <= 0) return fail(SVS_ERR_INVALID, "svs_index_assign: c must be >= 1, got %d", (int)c);
  if (nrows < 0) return fail(SVS_ERR_INVALID, "nrows must be >= 0");   // (reported ahead of the vectors' faults, as ever)
  if (!vectors) return fail(SVS_ERR_INVALID, "null vectors");
  if (c > SVS_ASSIGN_MAX_VECTORS)
    return fail(SVS_ERR_UNSUPPORTED, "svs_index_assign: %d vectors; a call takes at most %d", (int)c, SVS_ASSIGN_MAX_VECTORS);
  if (nrows == 0) {
    if (out_counts) memset(out_counts, 0, (size_t)c * sizeof(int64_t));
    return SVS_OK;
  }
  int64_t r0;
  int rc = label_range(idx, "svs_index_assign", row0, nrows, &r0);
  if (rc != SVS_OK) return rc;
  if (!out_best && !out_scores && !out_counts && !vector_labels) return SVS_OK;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const cx = fr.c;
  const size_t vec_bytes = (size_t)c * idx->ld * elem_bytes(idx);
  if ((rc = cx->as_vec.grow(vec_bytes)) != SVS_OK) return rc;
  if (idx->dtype == SVS_DTYPE_FP8 && (rc = cx->as_vec_scales.grow((size_t)c)) != SVS_OK) return rc;
  if (out_best && (rc = cx->as_best.grow((size_t)nrows)) != SVS_OK) return rc;
  if (out_scores && (rc = cx->as_score.grow((size_t)nrows)) != SVS_OK) return rc;
  if (out_counts && (rc = cx->as_cnt.grow((size_t)c)) != SVS_OK) return rc;
  if (vector_labels && ((rc = cx->lab_set_dev.grow((size_t)c)) != SVS_OK || (rc = cx->lab_set_pin.grow((size_t)c)) != SVS_OK)) return rc;
  if ((rc = cx->q_dev.grow((size_t)c * d)) != SVS_OK || (rc = cx->q_pin.grow((size_t)c * d)) != SVS_OK) return rc;
  // the column last: a call that fails above has allocated none
  if (vector_labels && (rc = column_ensure(idx, 0, "svs_index_assign")) != SVS_OK) return rc;
  hipStream_t st = fr.stream();
  // ---- the vectors as stored rows: the rows' own ingest path into the context's image
  if ((rc = upload_queries(cx, vectors, (size_t)c * d, st)) != SVS_OK) return rc;
  if (idx->dtype == SVS_DTYPE_F32 && idx->ld != d) HIP_TRY(hipMemsetAsync(cx->as_vec, 0, vec_bytes, st));
  const unsigned iblocks = idx->dtype == SVS_DTYPE_FP8 ? (unsigned)((c + 3) / 4)
                                                       : (unsigned)std::min<size_t>(((size_t)c * idx->ld + 255) / 256, 2048);
  HIP_TRY(ingest_rows_into(idx, cx->as_vec.p, cx->as_vec_scales.p, cx->q_dev, c, d, 0, hipMemcpyDeviceToDevice, iblocks, st));
  if (vector_labels) {
    memcpy(cx->lab_set_pin, vector_labels, (size_t)c * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(cx->lab_set_dev, cx->lab_set_pin, (size_t)c * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  if (out_counts) HIP_TRY(hipMemsetAsync(cx->as_cnt, 0, (size_t)c * sizeof(unsigned long long), st));
  // ---- one launch over the range (svs_index_set_timing: a span around it, read by svs_internal_assign_kernel_ms)
  const TimedSpan span(idx->timing.load() > 0);
  span.begin(st);
  launch_record("assign_rows_kernel", nrows, c);
  const uint32_t* const k_lab = vector_labels ? cx->lab_set_dev.p : nullptr;
  int32_t* const k_best = out_best ? cx->as_best.p : nullptr;
  float* const k_score = out_scores ? cx->as_score.p : nullptr;
  uint32_t* const k_col = vector_labels ? idx->cols[0] : nullptr;
  unsigned long long* const k_cnt = out_counts ? cx->as_cnt.p : nullptr;
  for_store_dtype(idx, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (c <= assign_sweep(1)) launch_assign_na<DT, 1>(idx, cx, c, r0, nrows, k_lab, k_best, k_score, k_col, k_cnt, st);
    else launch_assign_na<DT, 4>(idx, cx, c, r0, nrows, k_lab, k_best, k_score, k_col, k_cnt, st);
  });
  span.end(st);
  rc = read_back(fr, "assign", {{out_best, cx->as_best.p, (size_t)nrows * sizeof(int32_t)},
                                {out_scores, cx->as_score.p, (size_t)nrows * sizeof(float)},
                                {out_counts, cx->as_cnt.p, (size_t)c * sizeof(int64_t)}});
  if (rc == SVS_OK) g_assign_kernel_ms = span.ms();
  return rc;
}

int32_t svs_internal_assign_kernel_ms(double* out) { return report_ms(out, g_assign_kernel_ms); }

// ---- svs_index_label_sums (label_sums.h)
static_assert(SVS_LABEL_SUMS_CHUNK == LS_CHUNK, "the chunk length is part of the sum's definition");

int32_t svs_index_label_sums(svs_index* idx, const uint32_t* labels, int32_t nlabels, int64_t row0, int64_t nrows,
                             const uint32_t* row_labels, double* out_sums, int64_t* out_counts) {
  launch_reset();
  g_label_sums_kernel_ms = -1.0;   // (a call that fails or records nothing leaves no earlier call's time behind)
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // a reader like every search: one column, one bitmap for the whole call
  // ---- everything is validated before anything is written, allocated or launched
  if (idx->n == 0 || idx->d == 0) return fail(SVS_ERR_SHAPE, "svs_index_label_sums: the index is empty");
  // (the list holds local rows as u32 and a strip prefix is a u32: ensure_capacity admits at most 2^32 - 1 rows per handle)
  if (idx->n > 0xffffffffll) return fail(SVS_ERR_UNSUPPORTED, "svs_index_label_sums: %lld rows; a handle holds fewer than 2^32", (long long)idx->n);
  int64_t r0;
  int rc = LabelSet::check(labels, nlabels);
  if (rc != SVS_OK || (rc = label_range(idx, "svs_index_label_sums", row0, nrows, &r0)) != SVS_OK) return rc;
  LabelSet ls;
  if ((rc = ls.build("svs_index_label_sums", labels, nlabels)) != SVS_OK) return rc;
  const int nset = ls.nset, d = idx->d;
  if (nset == 0 || (!out_sums && !out_counts)) return SVS_OK;
  if (nrows == 0) {
    if (out_sums) std::fill(out_sums, out_sums + (size_t)nlabels * d, 0.0);
    if (out_counts) memset(out_counts, 0, (size_t)nlabels * sizeof(int64_t));
    return SVS_OK;
  }
  if (out_sums && (rc = check_gather_rows(idx, "svs_index_label_sums")) != SVS_OK) return rc;
  const int64_t nstrips = (nrows + LS_STRIP - 1) / LS_STRIP;
  const int64_t bound = (nrows + LS_CHUNK - 1) / LS_CHUNK + nset;   // chunks never cross a label: at most one ragged chunk each
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  if ((rc = c->ls_hist.grow((size_t)nstrips * nset)) != SVS_OK || (rc = c->ls_tot.grow(3 * (size_t)LB_MAX_SET + 1)) != SVS_OK ||
      (rc = c->ls_cnt_pin.grow((size_t)nset)) != SVS_OK)
    return rc;
  if (row_labels && (rc = c->ls_lab.grow((size_t)nrows)) != SVS_OK) return rc;
  if (out_sums && ((rc = c->ls_list.grow((size_t)nrows)) != SVS_OK || (rc = c->ls_table.grow((size_t)bound)) != SVS_OK ||
                   (rc = c->ls_part.grow((size_t)bound * d)) != SVS_OK || (rc = c->ls_out.grow((size_t)nset * d)) != SVS_OK ||
                   (rc = c->ls_out_pin.grow((size_t)nset * d)) != SVS_OK))
    return rc;
  hipStream_t st = fr.stream();
  LabelFilter f;
  if ((rc = ls.stage(idx, c, st, &f)) != SVS_OK) return rc;
  if (row_labels) HIP_TRY(hipMemcpyAsync(c->ls_lab, row_labels, (size_t)nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const LsRange g{r0, nrows, row_labels ? c->ls_lab.p : nullptr};
  unsigned long long* const tot = c->ls_tot.p;
  unsigned long long* const lbase = tot + LB_MAX_SET;
  unsigned long long* const cbase = tot + 2 * LB_MAX_SET;
  // ---- 1, 2: the strips' histogram and its scan; a count-only call ends here
  launch_record("label_sums_hist_kernel", nrows, nset);
  hipLaunchKernelGGL(label_sums_hist_kernel, dim3((unsigned)nstrips), dim3(LS_THREADS), 0, st, f, g, c->ls_hist.p);
  launch_record("label_sums_scan_kernel", nrows, nset);
  hipLaunchKernelGGL(label_sums_scan_kernel, dim3((unsigned)nset), dim3(LS_THREADS), 0, st, c->ls_hist.p, nstrips, nset, tot);
  const TimedSpan span(out_sums && idx->timing.load() > 0);
  if (out_sums) {
    // ---- 3, 4: the plan and the label-major list, on the device: no host wait before the sums
    launch_record("label_sums_plan_kernel", nrows, nset);
    hipLaunchKernelGGL(label_sums_plan_kernel, dim3(1), dim3(LS_PLAN_THREADS), 0, st, (const unsigned long long*)tot, nset, lbase, cbase,
                       c->ls_table.p, bound);
    launch_record("label_sums_scatter_kernel", nrows, nset);
    hipLaunchKernelGGL(label_sums_scatter_kernel, dim3((unsigned)nstrips), dim3(LS_THREADS), 0, st, f, g, (const uint32_t*)c->ls_hist.p,
                       (const unsigned long long*)lbase, (const unsigned long long*)tot, c->ls_list.p, nrows);
    // ---- 5, 6: chunk sums and fold (svs_index_set_timing: a span around them, read by svs_internal_label_sums_kernel_ms)
    span.begin(st);
    launch_record("label_sums_chunk_kernel", nrows, nset);
    for_store_dtype(idx, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      hipLaunchKernelGGL((label_sums_chunk_kernel<DT>), dim3((unsigned)bound, (unsigned)((ld16 + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS),
                         0, st, (const u32x4*)idx->rows, ld16, (const float*)idx->row_scales, idx->n, d, (const LsChunk*)c->ls_table.p,
                         (const uint32_t*)c->ls_list.p, nrows, c->ls_part.p);
    });
    launch_record("label_sums_fold_kernel", nrows, nset);
    hipLaunchKernelGGL(label_sums_fold_kernel, dim3((unsigned)((d + LS_FOLD_THREADS - 1) / LS_FOLD_THREADS), (unsigned)nset),
                       dim3(LS_FOLD_THREADS), 0, st, (const double*)c->ls_part.p, (const unsigned long long*)tot,
                       (const unsigned long long*)cbase, d, bound, c->ls_out.p);
    span.end(st);
  }
  rc = read_back(fr, "label_sums", {{c->ls_cnt_pin.p, tot, (size_t)nset * sizeof(unsigned long long)},
                                    {out_sums ? c->ls_out_pin.p : nullptr, c->ls_out.p, (size_t)nset * d * sizeof(double)}});
  if (rc != SVS_OK) return rc;
  g_label_sums_kernel_ms = span.ms();
  unsigned long long seen = 0;
  for (int s = 0; s < nset; ++s) {
    if (c->ls_cnt_pin[s] > (unsigned long long)nrows - seen)
      return fail(SVS_ERR_DEVICE, "label_sums: the histogram counted more than the range's %lld rows", (long long)nrows);
    seen += c->ls_cnt_pin[s];
  }
  // ---- the device worked on the sorted distinct set: every position of the caller's gets its label's answer
  for (int32_t j = 0; j < nlabels; ++j) {
    const size_t s = ls.slot_of(labels[j]);
    if (out_sums) memcpy(out_sums + (size_t)j * d, c->ls_out_pin + s * d, (size_t)d * sizeof(double));
    if (out_counts) out_counts[j] = (int64_t)c->ls_cnt_pin[s];
  }
  return SVS_OK;
}

int32_t svs_internal_label_sums_kernel_ms(double* out) { return report_ms(out, g_label_sums_kernel_ms); }

// The similarity matrices of one block of queries: 64 MiB, i.e. 16 queries at fetch_k = SVS_DIVERSE_MAX_FETCH (4 MiB each)
// and every query of most calls at the usual 32-256 candidates; a block costs two launches and no host wait.
constexpr size_t DIVERSE_G_BUDGET = (size_t)64 << 20;
static_assert(SVS_DIVERSE_MAX_FETCH == DV_MAX_FETCH, "the pick kernel's LDS arrays hold SVS_DIVERSE_MAX_FETCH candidates");

int32_t svs_index_search_diverse(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, int32_t fetch_k,
                                 float lambda_mult, float* out_scores, int64_t* out_rows, float* out_redundancy, int32_t* out_count) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  // ---- everything is validated before anything is written or launched
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  if (!(lambda_mult >= 0.f && lambda_mult <= 1.f))
    return fail(SVS_ERR_INVALID, "svs_index_search_diverse: lambda_mult must lie in [0, 1], got %g", (double)lambda_mult);
  if (k > 0 && fetch_k <= 0) return fail(SVS_ERR_INVALID, "svs_index_search_diverse: fetch_k must be >= 1, got %d", (int)fetch_k);
  if (fetch_k > 0 && fetch_k < k)
    return fail(SVS_ERR_INVALID, "svs_index_search_diverse: fetch_k (%d) is smaller than k (%d)", (int)fetch_k, (int)k);
  if (fetch_k > SVS_DIVERSE_MAX_FETCH)
    return fail(SVS_ERR_UNSUPPORTED, "svs_index_search_diverse: fetch_k %d; at most %d candidates are re-ranked", (int)fetch_k,
                SVS_DIVERSE_MAX_FETCH);
  const bool work = nq > 0 && k > 0;
  if (work && (!out_scores || !out_rows || !out_count)) return fail(SVS_ERR_INVALID, "null output");
  const int64_t live = idx->n - (int64_t)idx->dead_list.size();
  const int c = (int)std::min<int64_t>(std::max(fetch_k, 0), live);   // candidates per query
  const int count = std::min(std::max(k, 0), c);
  if (out_count) *out_count = count;
  if (!work || count == 0) return SVS_OK;
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const cx = fr.c;
  // ---- candidates: the ordinary host search at fetch_k, left in the context's pinned block (stride c)
  if ((rc = search_host_framed(idx, fr, queries, nq, d, c, c, nullptr, nullptr)) != SVS_OK) return rc;
  if (count == 1) {   // (k == 1 or c == 1) the best candidate: nothing behind the search
    for (int32_t q = 0; q < nq; ++q) {
      out_scores[(size_t)q * k] = cx->out_s_pin[(size_t)q * c];
      out_rows[(size_t)q * k] = cx->out_r_pin[(size_t)q * c];
      if (out_redundancy) out_redundancy[(size_t)q * k] = -std::numeric_limits<float>::infinity();
    }
    return SVS_OK;
  }
  const size_t cc = (size_t)c * (size_t)c;
  // (and at most 32,768 queries: a block's queries are the grid's y dimension)
  const int qb = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)nq, 32768), DIVERSE_G_BUDGET / (cc * sizeof(float))));
  const size_t on = (size_t)nq * (size_t)count;
  if ((rc = cx->dv_G.grow((size_t)qb * cc)) != SVS_OK) return rc;
  if ((rc = cx->dv_s_pin.grow(on)) != SVS_OK || (rc = cx->dv_r_pin.grow(on)) != SVS_OK || (rc = cx->dv_red_pin.grow(on)) != SVS_OK) return rc;
  const hipStream_t st = fr.stream();
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  const int nt = (c + DV_TILE - 1) / DV_TILE;
  const u32x4* M = (const u32x4*)idx->rows;
  const float oml = 1.0f - lambda_mult;
  // Block by block on the context's stream (the scratch is reused in stream order); one wait for the whole call
  for (int q0 = 0; q0 < nq; q0 += qb) {
    const int nb = std::min(qb, nq - q0);
    // (the candidates stay in the pinned, device-visible block the search wrote them to: a workgroup of the Gram kernel
    //  reads 128 row numbers over the bus, the pick kernel c scores and rows; copying them into HBM first measured the same)
    const int64_t* cand_r = cx->out_r_pin + (size_t)q0 * c;
    const float* cand_s = cx->out_s_pin + (size_t)q0 * c;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)nb);
    launch_record("diverse_gram_kernel", c, nb);
    for_store_dtype(idx, [&](auto dt) {
      hipLaunchKernelGGL(diverse_gram_kernel<dt()>, grid, dim3(DV_THREADS), 0, st, M, ld16, (const float*)idx->row_scales, cand_r,
                         c, idx->row_offset, idx->n, nt, cx->dv_G.p);   // (row_scales: null unless fp8)
    });
    launch_record("diverse_pick_kernel", c, nb);
    hipLaunchKernelGGL(diverse_pick_kernel, dim3((unsigned)nb), dim3(DV_PICK_THREADS), 0, st, cand_s, cand_r,
                       (const float*)cx->dv_G.p, c, count, lambda_mult, oml,
                       cx->dv_s_pin + (size_t)q0 * count, cx->dv_r_pin + (size_t)q0 * count, cx->dv_red_pin + (size_t)q0 * count);
  }
  if ((rc = fr.close("search_diverse")) != SVS_OK) return rc;
  deliver_strided(out_scores, k, cx->dv_s_pin.p, count, nq);
  deliver_strided(out_rows, k, cx->dv_r_pin.p, count, nq);
  if (out_redundancy) deliver_strided(out_redundancy, k, cx->dv_red_pin.p, count, nq);
  return SVS_OK;
}

int32_t svs_index_search_segments(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, const int64_t* rows,
                                  const int64_t* seg_begin, const int32_t* seg_query, int32_t nseg, float* out_scores,
                                  int64_t* out_rows, int32_t* out_counts) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  // ---- everything is validated before anything is written or launched
  int rc = check_query_args(idx, queries, nq, d);
  if (rc != SVS_OK) return rc;
  if (nseg < 0) return fail(SVS_ERR_INVALID, "nseg must be >= 0");
  if (!seg_query && nseg != nq)
    return fail(SVS_ERR_INVALID, "svs_index_search_segments: %d segments for %d queries and no seg_query", nseg, nq);
  if (nseg == 0) return SVS_OK;
  if (!seg_begin) return fail(SVS_ERR_INVALID, "null seg_begin");
  if (seg_begin[0] != 0) return fail(SVS_ERR_INVALID, "seg_begin[0] must be 0, not %lld", (long long)seg_begin[0]);
  for (int32_t s = 0; s < nseg; ++s) {
    if (seg_begin[s + 1] < seg_begin[s])
      return fail(SVS_ERR_INVALID, "seg_begin decreases at segment %d (%lld after %lld)", s, (long long)seg_begin[s + 1], (long long)seg_begin[s]);
    if (seg_query && (seg_query[s] < 0 || seg_query[s] >= nq))
      return fail(SVS_ERR_INVALID, "segment %d: query %d outside [0, %d)", s, seg_query[s], nq);
  }
  const int64_t total = seg_begin[nseg];
  if (total > 0 && !rows) return fail(SVS_ERR_INVALID, "null row list");
  const int64_t lo = idx->row_offset, n = idx->n;
  std::vector<uint8_t> ascending;
  std::vector<int64_t> m_of, off_of, res_of;   // per segment: live rows, where its list begins in S, its results in the result block
  std::vector<uint32_t> tmp, big;   // an unsorted segment's rows; the lists of the large segments, one after the other
  try {
    ascending.assign((size_t)nseg, 1);
    m_of.assign((size_t)nseg, 0);
    off_of.assign((size_t)nseg, -1);
    res_of.assign((size_t)nseg, 0);
  } catch (const std::bad_alloc&) {
    return fail(SVS_ERR_NOMEM, "out of host memory for %d segments", nseg);
  }
  for (int32_t s = 0; s < nseg; ++s)
    for (int64_t t = seg_begin[s]; t < seg_begin[s + 1]; ++t) {
      const int64_t r = rows[t] - lo;
      if (r < 0 || r >= n)
        return fail(SVS_ERR_INVALID, "segment %d: row %lld out of range [%lld, %lld)", s, (long long)rows[t], (long long)lo, (long long)(lo + n));
      if (t > seg_begin[s] && rows[t] <= rows[t - 1]) ascending[(size_t)s] = 0;
    }
  if (!out_counts) return fail(SVS_ERR_INVALID, "null out_counts");
  if (k > 0 && total > 0 && (!out_scores || !out_rows)) return fail(SVS_ERR_INVALID, "null output");
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  const int W = gather_rows_per_wave(idx);
  if (k > 0 && total > 0 && W == 0)
    return fail(SVS_ERR_UNSUPPORTED, "svs_index_search_segments: rows of %d bytes; the gather kernels take rows of up to 16 KiB", ld16 * 16);
  if (k <= 0 || total == 0) {
    for (int32_t s = 0; s < nseg; ++s) out_counts[s] = 0;
    return SVS_OK;
  }
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  // ---- host plan: S = the live rows of every segment, ascending inside it, as local u32 rows in pinned memory --
  // the small segments (1 .. SORT_CAP live rows) first, in segment order, then the large ones
  if ((rc = c->list_pin.grow((size_t)total)) != SVS_OK) return rc;
  uint32_t* S = c->list_pin;
  const uint8_t* dead = idx->dead_flag.data();
  int64_t small_rows = 0, max_small = 0, max_large = 0, n_small = 0, n_large = 0, large_out = 0;
  try {
    for (int32_t s = 0; s < nseg; ++s) {
      const int64_t b = seg_begin[s], nr = seg_begin[s + 1] - b;
      // (a segment that lists more than SORT_CAP rows may be large: it is built aside and placed once its size is known)
      const bool aside = nr > SORT_CAP;
      if (aside) big.resize(big.size() + (size_t)nr);
      uint32_t* dst = aside ? big.data() + (big.size() - (size_t)nr) : S + small_rows;
      const int64_t m = live_rows_ascending(rows + b, nr, lo, dead, ascending[(size_t)s] != 0, tmp, dst);
      m_of[(size_t)s] = m;
      if (aside && m <= SORT_CAP) {   // small after all
        memcpy(S + small_rows, dst, (size_t)m * sizeof(uint32_t));
        big.resize(big.size() - (size_t)nr);
      } else if (aside) {
        big.resize(big.size() - (size_t)(nr - m));
        ++n_large;
        max_large = std::max(max_large, m);
        large_out += std::min<int64_t>(k, m);
      }
      if (m >= 1 && m <= SORT_CAP) {
        small_rows += m;
        ++n_small;
        max_small = std::max(max_small, m);
      }
    }
  } catch (const std::bad_alloc&) {
    return fail(SVS_ERR_NOMEM, "out of host memory for a %lld-row list", (long long)total);
  }
  if (n_small == 0 && n_large == 0) {
    for (int32_t s = 0; s < nseg; ++s) out_counts[s] = 0;
    return SVS_OK;
  }
  const int64_t ntiles = seg_tile_plan(m_of.data(), seg_query, nseg, W, nullptr, 0, off_of.data(), nullptr);
  if (ntiles < 0)
    return fail(SVS_ERR_UNSUPPORTED, "svs_index_search_segments: the small segments list %lld live rows; one call takes fewer than 2^31",
                (long long)small_rows);
  if (!big.empty()) memcpy(S + small_rows, big.data(), big.size() * sizeof(uint32_t));
  const int64_t listed = small_rows + (int64_t)big.size();
  const int kk = (int)std::min<int64_t>(k, max_small);   // the small segments' result stride
  const size_t plan_n = (size_t)ntiles + (size_t)n_small;
  if ((rc = c->seg_plan_pin.grow(std::max<size_t>(plan_n, 1))) != SVS_OK || (rc = c->seg_plan_dev.grow(std::max<size_t>(plan_n, 1))) != SVS_OK) return rc;
  SegTile* tiles = c->seg_plan_pin;
  SegDesc* segs = reinterpret_cast<SegDesc*>(tiles + ntiles);
  (void)seg_tile_plan(m_of.data(), seg_query, nseg, W, tiles, ntiles, nullptr, nullptr);
  // the result block: rows (int64) of the small segments at stride kk, then of the large ones, count by count; the
  // scores (f32) behind them in the same order
  const size_t res_n = (size_t)n_small * (size_t)kk + (size_t)large_out;
  {
    int64_t j = 0, loff = small_rows, o = n_small * kk;
    for (size_t s = 0; s < (size_t)nseg; ++s) {
      const int64_t m = m_of[s], count = std::min<int64_t>(k, m);
      if (m > SORT_CAP) {   // (the large segments' lists lie behind the small ones', in segment order)
        off_of[s] = loff;
        res_of[s] = o;
        loff += m;
        o += count;
      } else if (m >= 1) {
        res_of[s] = j * kk;
        segs[j++] = SegDesc{(uint32_t)off_of[s], (uint32_t)m, (uint32_t)count, (uint32_t)s};
      }
    }
  }
  const size_t res_words = res_n + (res_n + 1) / 2;
  if ((rc = c->list_dev.grow((size_t)listed)) != SVS_OK) return rc;
  if ((rc = c->seg_res_dev.grow(res_words)) != SVS_OK || (rc = c->seg_res_pin.grow(res_words)) != SVS_OK) return rc;
  const int64_t small_stride = score_stride(small_rows), large_stride = score_stride(max_large);
  if ((rc = c->scores.grow((size_t)std::max(small_stride, large_stride))) != SVS_OK) return rc;
  bool window = false;
  for (int32_t s = 0; s < nseg && !window; ++s)
    window = m_of[(size_t)s] > SORT_CAP && select_path(m_of[(size_t)s], (int)std::min<int64_t>(k, m_of[(size_t)s])) == SelectPath::WINDOW;
  const hipStream_t st = fr.stream();
  if (window && (rc = grow_select_scratch(c, 1, st)) != SVS_OK) return rc;
  int64_t* res_r = c->seg_res_dev;
  float* res_s = reinterpret_cast<float*>(res_r + res_n);
  if ((rc = upload_queries(c, queries, (size_t)nq * (size_t)d, st)) != SVS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->list_dev, S, (size_t)listed * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (n_small) {
    HIP_TRY(hipMemcpyAsync(c->seg_plan_dev, tiles, plan_n * sizeof(SegTile), hipMemcpyHostToDevice, st));
    const SegTile* tiles_dev = c->seg_plan_dev;
    if ((rc = launch_gather_segments(idx, c, c->q_dev, nq, c->list_dev, tiles_dev, ntiles, small_rows, (int)n_small, c->scores, st)) != SVS_OK)
      return rc;
    launch_record("select_segments_kernel", small_rows, (int)n_small);
    hipLaunchKernelGGL(select_segments_kernel, dim3((unsigned)n_small), dim3(FINAL_THREADS), 0, st, (const float*)c->scores,
                       (const uint32_t*)c->list_dev, reinterpret_cast<const SegDesc*>(tiles_dev + ntiles), kk, lo, res_s, res_r);
  }
  // The large segments, one after the other behind the small ones' two kernels on the same stream, each the search
  // svs_index_search_rows makes over its one list: launch_gather re-stages its query into the buffers the small segments'
  // kernel read its queries from, and the scores are reused -- both in stream order, behind their readers.
  for (int32_t s = 0; s < nseg; ++s) {
    const int64_t m = m_of[(size_t)s], o = res_of[(size_t)s];
    if (m <= SORT_CAP) continue;
    const int sq = seg_query ? seg_query[s] : s;
    if ((rc = enqueue_list_search(idx, c, c->q_dev + (size_t)sq * d, 1, c->list_dev + off_of[(size_t)s], m, (int)std::min<int64_t>(k, m),
                                  res_s + o, res_r + o, st)) != SVS_OK)
      return rc;
  }
  if ((rc = fr.launched("search_segments")) != SVS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->seg_res_pin, c->seg_res_dev, res_n * sizeof(int64_t) + res_n * sizeof(float), hipMemcpyDeviceToHost, st));
  if ((rc = fr.wait()) != SVS_OK) return rc;
  // ---- delivery: the large segments' positions -> rows in the pinned block, every one checked; then count_s entries per
  // segment at the caller's stride k
  int64_t* pr = c->seg_res_pin;
  const float* ps = reinterpret_cast<const float*>(pr + res_n);
  for (size_t s = 0; s < (size_t)nseg; ++s)
    if (m_of[s] > SORT_CAP &&
        (rc = list_positions_to_rows(pr + res_of[s], (size_t)std::min<int64_t>(k, m_of[s]), S + off_of[s], m_of[s], lo, (int)s)) != SVS_OK)
      return rc;
  for (size_t s = 0; s < (size_t)nseg; ++s) {
    const size_t count = (size_t)std::min<int64_t>(k, m_of[s]);
    out_counts[s] = (int32_t)count;
    memcpy(out_scores + s * k, ps + res_of[s], count * sizeof(float));
    memcpy(out_rows + s * k, pr + res_of[s], count * sizeof(int64_t));
  }
  return SVS_OK;
}

// rows_as_queries_kernel: the f32 panel of nq listed rows (list_dev: local rows on the device) into `panel`
static void launch_rows_as_queries(const svs_index* idx, const uint32_t* list_dev, int nq, float* panel, hipStream_t st) {
  const int ld16 = (int)((size_t)idx->ld * elem_bytes(idx) / 16);
  const int epc = 16 / (int)elem_bytes(idx);
  const int64_t items = (int64_t)nq * ((idx->d + epc - 1) / epc);
  const unsigned blocks = (unsigned)std::min<int64_t>(4096, (items + NEIGHBORS_THREADS - 1) / NEIGHBORS_THREADS);
  launch_record("rows_as_queries_kernel", nq, nq);
  const u32x4* M = (const u32x4*)idx->rows;
  for_store_dtype(idx, [&](auto dt) {
    hipLaunchKernelGGL(rows_as_queries_kernel<dt()>, dim3(blocks), dim3(NEIGHBORS_THREADS), 0, st, M, ld16, (const float*)idx->row_scales,
                       list_dev, nq, idx->d, panel);
  });
}

// drop_self_kernel: nq results at stride count + 1 -> count entries each at stride count
static void launch_drop_self(const svs_index* idx, const float* in_s, const int64_t* in_r, const uint32_t* list_dev, int nq, int count,
                             float* out_s, int64_t* out_r, hipStream_t st) {
  constexpr int WPB = NEIGHBORS_THREADS / 64;
  launch_record("drop_self_kernel", count + 1, nq);
  hipLaunchKernelGGL(drop_self_kernel, dim3((unsigned)((nq + WPB - 1) / WPB)), dim3(NEIGHBORS_THREADS), 0, st, in_s, in_r, list_dev,
                     idx->row_offset, nq, count, out_s, out_r);
}

int32_t svs_index_neighbors(svs_index* idx, const int64_t* rows, int64_t nrows, int32_t k, float* out_scores, int64_t* out_rows,
                            int32_t* out_count) {
  launch_reset();
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  const int64_t lo = idx->row_offset, n = idx->n;
  // (the first offending row of the list decides the error: a tombstoned row in front of the first row out of range wins)
  for (int64_t t = 0; rows && t < nrows; ++t) {
    const int64_t r = rows[t] - lo;
    if (r < 0 || r >= n) break;
    if (idx->dead_flag[(size_t)r]) return fail(SVS_ERR_INVALID, "row %lld is tombstoned: it has no neighbours", (long long)rows[t]);
  }
  int rc = check_row_list(rows, nrows, lo, n, nullptr);
  if (rc != SVS_OK) return rc;
  const int64_t live = n - (int64_t)idx->dead_list.size();
  const int count = (int)std::min<int64_t>(std::max(k, 0), std::max<int64_t>(live - 1, 0));
  if (out_count) *out_count = count;
  if (nrows == 0 || count == 0) return SVS_OK;
  if (!out_scores || !out_rows) return fail(SVS_ERR_INVALID, "null output");
  if (idx->d == 0) return fail(SVS_ERR_SHAPE, "an index of dimension 0 has no scores");
  HostCall fr(idx);
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  const int kk = count + 1, d = idx->d;   // (kk <= live rows: the search's own count is kk)
  const int64_t B = SVS_NEIGHBORS_BLOCK;
  const int bmax = (int)std::min<int64_t>(B, nrows);
  const size_t on = (size_t)nrows * (size_t)count;
  if ((rc = c->nb_list_pin.grow((size_t)nrows)) != SVS_OK || (rc = c->nb_list_dev.grow((size_t)nrows)) != SVS_OK) return rc;
  if ((rc = c->q_dev.grow((size_t)bmax * d)) != SVS_OK) return rc;
  if ((rc = c->nb_s.grow((size_t)bmax * kk)) != SVS_OK || (rc = c->nb_r.grow((size_t)bmax * kk)) != SVS_OK) return rc;
  if ((rc = c->out_s_pin.grow(on)) != SVS_OK || (rc = c->out_r_pin.grow(on)) != SVS_OK) return rc;
  for (int64_t t = 0; t < nrows; ++t) c->nb_list_pin[t] = (uint32_t)(rows[t] - lo);
  HIP_TRY(hipMemcpyAsync(c->nb_list_dev, c->nb_list_pin, (size_t)nrows * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  // Block by block on the context's stream: panel, the ordinary search at count + 1 into device scratch, self dropped
  // into the pinned (device-visible) output.  One wait for the whole call.
  const int variant = idx->variant.load();
  for (int64_t b0 = 0; b0 < nrows; b0 += B) {
    const int nb = (int)std::min<int64_t>(B, nrows - b0);
    const uint32_t* list = c->nb_list_dev + b0;
    SearchPlan plan;
    if ((rc = plan_search(idx, c, nb, kk, kk, st, true, variant, &plan)) != SVS_OK) return rc;
    launch_rows_as_queries(idx, list, nb, c->q_dev, st);
    if ((rc = enqueue_prefix(idx, c, plan, c->q_dev, st)) == SVS_OK) rc = enqueue_main(idx, c, plan, c->q_dev, c->nb_s, c->nb_r, st);
    if (rc != SVS_OK) {
      plan_abandon(idx, plan);
      return rc;
    }
    launch_drop_self(idx, c->nb_s, c->nb_r, list, nb, count, c->out_s_pin + (size_t)b0 * count, c->out_r_pin + (size_t)b0 * count, st);
  }
  if ((rc = fr.close("neighbors")) != SVS_OK) return rc;
  // Overflowed positions: rerun_overflowed block by block, so in the groups search_host forms for the block (the same
  // kernels, the same bits).  There is no host copy of the queries: the group's rows are turned into a panel of its own,
  // and the search's count + 1 results per row go through drop_self like the block's.
  auto stage = [&](const int64_t* grp, int m) -> int {
    int rc;
    if ((rc = c->nb_redo_pin.grow(REDO_BATCH)) != SVS_OK || (rc = c->nb_redo_dev.grow(REDO_BATCH)) != SVS_OK) return rc;
    if ((rc = c->nb_redo_q.grow((size_t)REDO_BATCH * d)) != SVS_OK) return rc;
    for (int j = 0; j < m; ++j) c->nb_redo_pin[j] = c->nb_list_pin[grp[j]];
    HIP_TRY(hipMemcpyAsync(c->nb_redo_dev, c->nb_redo_pin, (size_t)m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    launch_rows_as_queries(idx, c->nb_redo_dev, m, c->nb_redo_q, st);
    return SVS_OK;
  };
  auto finish = [&](int m) { launch_drop_self(idx, c->nb_s, c->nb_r, c->nb_redo_dev, m, count, c->redo_s_pin, c->redo_r_pin, st); };
  int n_redo = 0;
  for (int64_t b0 = 0; b0 < nrows; b0 += B)
    if ((rc = rerun_overflowed(idx, fr, b0, std::min<int64_t>(b0 + B, nrows), count, kk, c->nb_redo_q, c->nb_s, c->nb_r, stage, finish, &n_redo)) != SVS_OK) return rc;
  g_host_phase[5] = (double)n_redo;
  deliver_results(c, nrows, count, k, out_scores, out_rows);
  return SVS_OK;
}

int32_t svs_index_top_pairs(svs_index* idx, int32_t k, float* out_scores, int64_t* out_i, int64_t* out_j,
                            int32_t* out_count) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  launch_reset();
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  const int64_t n = idx->n;
  const int64_t np = score_stride(n);
  const int64_t n_live = n - (int64_t)idx->dead_list.size();
  const int64_t pairs = n_live * (n_live - 1) / 2;
  const int count = (int)std::min<int64_t>(std::max(k, 0), pairs);
  if (out_count) *out_count = count;
  if (count == 0) return SVS_OK;
  if (!out_scores || !out_i || !out_j) return fail(SVS_ERR_INVALID, "null output");
  HostCall fr(idx);
  if (const int rc = fr.open(); rc != SVS_OK) return rc;
  // Small corpora: materialise n x n like the reference (src/svs/kb.py:1651).  Past n^2 = 2^32 scores
  // (or with variant 1, for A/B and tests): tiled GEMM with the i < j mask and a threshold in the
  // fused epilogue, nothing materialised but a prefix block.
  // (Up to GQ rows always: the one query chunk of such a corpus would take the 16-query kernels, which have no pair mode
  //  -- under variant 1 they returned (i, i) and both (i, j) and (j, i).)
  const int variant = idx->variant.load();   // (once: every chunk of either path takes its route under this value)
  if (n * np <= 0xffffffffll && (variant != VARIANT_GEMV_PERSISTENT_R1 || n <= GQ))
    return top_pairs_materialised(idx, fr, variant, n, count, out_scores, out_i, out_j);
  return top_pairs_tiled(idx, fr, variant, count, out_scores, out_i, out_j);
}

int32_t svs_index_debug_dequant(svs_index* idx, int64_t row0, int64_t nrows, float* out) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  if (row0 < 0 || nrows < 0 || row0 + nrows > idx->n) return fail(SVS_ERR_INVALID, "row range out of bounds");
  if (nrows == 0 || idx->d == 0) return SVS_OK;
  HIP_TRY(hipSetDevice(idx->device));
  { int rc = staging_wait(idx); if (rc != SVS_OK) return rc; }
  const size_t cnt = (size_t)nrows * idx->d;
  if (idx->dtype == SVS_DTYPE_F32) {
    HIP_TRY(hipMemcpy2D(out, (size_t)idx->d * sizeof(float), (const float*)idx->rows + row0 * idx->ld,
                        (size_t)idx->ld * sizeof(float), (size_t)idx->d * sizeof(float), (size_t)nrows, hipMemcpyDeviceToHost));
    return SVS_OK;
  }
  float* tmp = nullptr;
  HIP_TRY(hipMalloc((void**)&tmp, cnt * sizeof(float)));
  (void)dequant_rows_to(idx, row0, nrows, tmp, 0);   // (f16 / fp8: a kernel launch, which reports nothing here)
  hipError_t e = hipMemcpy(out, tmp, cnt * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(SVS_ERR_DEVICE, "dequant read-back: %s", hipGetErrorString(e));
  return SVS_OK;
}

int32_t svs_index_debug_query(svs_index* idx, const float* query, int32_t d, float* out) {
  if (!idx || !query || !out) return fail(SVS_ERR_INVALID, "null argument");
  if (d != idx->d) return fail(SVS_ERR_SHAPE, "query dim %d != index dim %d", d, idx->d);
  if (idx->dtype == SVS_DTYPE_F32 || d == 0) {
    memcpy(out, query, (size_t)d * sizeof(float));
    return SVS_OK;
  }
  // build a one-row index of the same dtype from the query and read it back: the
  // row path and the query path share their rounding / quantisation kernels
  svs_index* tmp = nullptr;
  int rc = svs_index_create(query, 1, d, idx->dtype, idx->device, 0, &tmp);
  if (rc != SVS_OK) return rc;
  rc = svs_index_debug_dequant(tmp, 0, 1, out);
  svs_index_release(tmp);
  return rc;
}

// The bytes of an image as they lie in HBM (internal.h): device-to-host copies only, no kernel, so that the tests read
// what ingest wrote without going through the library's own decoders.
int32_t svs_internal_stored_image(svs_index* idx, int32_t what, int64_t row0, int64_t nrows, void* out, int64_t capacity_bytes) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  if (what < 0 || what > 2) return fail(SVS_ERR_INVALID, "unknown image %d", what);
  HIP_TRY(hipSetDevice(idx->device));
  { int rc = staging_wait(idx); if (rc != SVS_OK) return rc; }
  std::shared_lock<std::shared_mutex> geo(idx->rw);   // (appends, commits and compactions take it exclusively: n and the pointers stand still)
  const void* base = what == 0 ? idx->rows : (what == 1 ? (const void*)idx->row_scales : idx->shadow);
  if (what == 1 && idx->dtype != SVS_DTYPE_FP8) return fail(SVS_ERR_UNSUPPORTED, "only an fp8 index has row scales");
  if (what == 2 && !idx->shadow) return fail(SVS_ERR_UNSUPPORTED, "the index has no half shadow");
  if (row0 < 0 || nrows < 0 || row0 > idx->n || nrows > idx->n - row0) return fail(SVS_ERR_INVALID, "row range out of bounds");
  const size_t row_b = what == 0 ? (size_t)idx->ld * elem_bytes(idx) : (what == 1 ? sizeof(float) : (size_t)idx->ld * sizeof(_Float16));
  const size_t bytes = (size_t)nrows * row_b;
  if (capacity_bytes < 0 || (uint64_t)capacity_bytes < bytes)
    return fail(SVS_ERR_INVALID, "the image takes %zu bytes, the buffer holds %lld", bytes, (long long)capacity_bytes);
  if (bytes == 0) return SVS_OK;
  HIP_TRY(hipMemcpy(out, (const char*)base + (size_t)row0 * row_b, bytes, hipMemcpyDeviceToHost));
  return SVS_OK;
}

int32_t svs_index_set_timing(svs_index* idx, int32_t enable) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  idx->timing.store(enable > 0 ? enable : 0);
  idx->timing_seq.store(0);
  return SVS_OK;
}

int32_t svs_index_get_timing(svs_index* idx, svs_timing_t* out) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(idx->device));
  std::vector<EvTriple> evs;
  {
    std::lock_guard<std::mutex> lk(idx->mu);
    evs.swap(idx->evs);
  }
  out->score_ms_sum = 0;
  out->select_ms_sum = 0;
  out->launches = 0;
  out->dominant_ms_sum = 0;
  int rc = SVS_OK;
  for (auto& t : evs) {
    float a = 0, b = 0;
    hipError_t e = hipEventSynchronize(t.e2);
    if (e == hipSuccess) e = hipEventElapsedTime(&a, t.e0, t.e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&b, t.e1, t.e2);
    float dm = a;
    if (e == hipSuccess && t.d0 && t.d1) e = hipEventElapsedTime(&dm, t.d0, t.d1);
    if (e == hipSuccess) {
      out->score_ms_sum += a;
      out->select_ms_sum += b;
      out->dominant_ms_sum += dm;
      out->launches++;
    } else {
      rc = fail(SVS_ERR_DEVICE, "timing events: %s", hipGetErrorString(e));
    }
    ev_destroy(t);
  }
  return rc;
}

int32_t svs_internal_tune(int32_t what, int64_t value) {
  switch (what) {
    case 0: if (value < 1) break; g_tune_prefix_div.store(value); return SVS_OK;
    case 1: if (value < 0 || value > 1) break; g_tune_upload.store(value); return SVS_OK;
    case 2: if (value < 0 || value > 1) break; g_tune_spread.store(value); return SVS_OK;
    case 3: if (value < 0 || value > 1) break; g_tune_refuse_shadow.store(value); return SVS_OK;
    case 4: if (value < 0 || value > 1) break; g_tune_handover.store(value); return SVS_OK;
    case 5: if (value < 1 || value > SHARE_MAX) break; g_tune_share.store(value); return SVS_OK;
    case 6: if (value < 0 || value > 2) break; g_tune_thin.store(value); return SVS_OK;
    case 7: if (value != BL_ATOMIC && value != BL_PARTIALS) break; g_tune_by_label_cross.store(value); return SVS_OK;
    case 8: if (value < 0 || value > 2) break; g_tune_combine_route.store(value); return SVS_OK;
    default: break;
  }
  return fail(SVS_ERR_INVALID, "svs_internal_tune(%d, %lld): unknown knob or value", what, (long long)value);
}

int32_t svs_internal_host_phases(double* out, int32_t n) {
  for (int i = 0; i < n && i < 6; ++i) out[i] = g_host_phase[i];
  return SVS_OK;
}

int64_t svs_internal_redo_groups(const int64_t* res_rows, int32_t count, int64_t q0, int64_t q1, int32_t max, int64_t* positions,
                                 int64_t* sizes, int64_t* n_groups) {
  if (!res_rows || count < 1 || q0 < 0 || q1 < q0 || max < 1 || max > REDO_BATCH || !positions || !sizes || !n_groups)
    return fail(SVS_ERR_INVALID, "svs_internal_redo_groups: 0 <= q0 <= q1, count >= 1, 1 <= max <= %d", REDO_BATCH);
  int64_t found = 0, groups = 0;
  while (const int m = next_redo_group(res_rows, count, &q0, q1, max, positions + found)) {
    sizes[groups++] = m;
    found += m;
  }
  *n_groups = groups;
  return found;
}

int64_t svs_internal_live_rows(const int64_t* rows, int64_t nrows, int64_t row_offset, int64_t n, const uint8_t* dead_flags, uint32_t* out,
                               int64_t cap) {
  if (n < 0 || n > ((int64_t)1 << 32) || cap < nrows || (nrows > 0 && (!dead_flags || !out)))
    return fail(SVS_ERR_INVALID, "svs_internal_live_rows: nrows <= cap, 0 <= n <= 2^32, no null array");
  bool ascending;
  if (const int rc = check_row_list(rows, nrows, row_offset, n, &ascending); rc != SVS_OK) return rc;
  try {
    std::vector<uint32_t> tmp;
    return live_rows_ascending(rows, nrows, row_offset, dead_flags, ascending, tmp, out);
  } catch (const std::bad_alloc&) {
    return fail(SVS_ERR_NOMEM, "out of host memory for a %lld-row list", (long long)nrows);
  }
}

int32_t svs_internal_single_route(int32_t dtype, int32_t d, int32_t variant, int32_t screen, char* kernel, int32_t cap, int32_t* flags) {
  svs_index shape;   // (never sees a device: the route and the launchers' names depend on dtype, d and ld alone)
  shape.dtype = dtype; shape.d = d; shape.ld = choose_ld(d, dtype);
  if (dtype < SVS_DTYPE_F32 || dtype > SVS_DTYPE_FP8 || d < 1 || variant < VARIANT_DEFAULT || variant > VARIANT_LAST || !kernel || cap < 1 ||
      !flags || (screen && !shadow_eligible(&shape)))
    return fail(SVS_ERR_INVALID, "svs_internal_single_route: no index of dtype %d, d %d, variant %d, screen %d", dtype, d, variant, screen);
  const SingleRoute r = single_route(&shape, variant, screen != 0);
  const Ctx ctx;
  const char* name = nullptr;
  const int rc = launch_route(&shape, &ctx, r, nullptr, nullptr, nullptr, PassOpts{nullptr, nullptr, 0, false, &name});
  if (rc != SVS_OK) return rc;
  snprintf(kernel, (size_t)cap, "%s", name);
  *flags = (r.shares ? 1 : 0) | (r.query == SingleRoute::PADDED ? 2 : 0);
  return SVS_OK;
}

int32_t svs_internal_batch_route(int32_t dtype, int32_t d, int32_t variant, int32_t nq, int64_t n_rows, int32_t flags, char* kernel, int32_t cap,
                                 int32_t* info) {
  if (dtype < SVS_DTYPE_F32 || dtype > SVS_DTYPE_FP8 || d < 1 || variant < VARIANT_DEFAULT || variant > VARIANT_LAST || nq < 2 || n_rows < 1 ||
      (flags & ~3) || !kernel || cap < 1 || !info)
    return fail(SVS_ERR_INVALID, "svs_internal_batch_route: no batch of %d queries on an index of dtype %d, d %d, variant %d", nq, dtype, d, variant);
  svs_index shape;   // (never sees a device: the route and the launchers' names depend on dtype, d and ld alone)
  shape.dtype = dtype; shape.d = d; shape.ld = choose_ld(d, dtype);
  const BatchRoute r = batch_route(&shape, variant, nq);
  Ctx ctx;
  static uint32_t fused_state;   // (its address only: a non-null FuseLaunch::state selects the fused forms)
  FuseLaunch fl{};
  if (flags & 1) fl.state = &fused_state;
  fl.pairs.on = (flags >> 1) & 1;
  const char* name = nullptr;
  const int rc = launch_batch(&shape, &ctx, r, nullptr, n_rows, nullptr, 0, fl, nullptr, &name);
  if (rc != SVS_OK) return rc;
  snprintf(kernel, (size_t)cap, "%s", name);
  info[0] = r.family; info[1] = r.tile; info[2] = r.rows();
  return SVS_OK;
}

int32_t svs_internal_last_launches(const char** kernels, int64_t* rows, int32_t* nq, int32_t cap) {
  for (int i = 0; i < cap && i < g_nlaunch && i < LAUNCH_REC_CAP; ++i) {
    if (kernels) kernels[i] = g_launch[i].kernel;
    if (rows) rows[i] = g_launch[i].rows;
    if (nq) nq[i] = g_launch[i].nq;
  }
  return g_nlaunch;
}

int32_t svs_index_set_screen(svs_index* idx, int32_t mode) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (mode != 0 && mode != 1) return fail(SVS_ERR_INVALID, "svs_index_set_screen: mode %d (0 = off, 1 = automatic)", mode);
  RefGuard guard(idx);
  std::unique_lock<std::shared_mutex> geo(idx->rw);
  HIP_TRY(hipSetDevice(idx->device));
  int rc = staging_wait(idx);
  if (rc != SVS_OK) return rc;
  idx->screen_mode.store(mode);
  idx->geo_epoch.fetch_add(1);
  if (mode == 0) {
    HIP_TRY(hipDeviceSynchronize());   // searches enqueued by the device API may still read the shadow
    shadow_free(idx);
    return SVS_OK;
  }
  idx->shadow_gave_up = false;
  if (!idx->shadow && idx->n > 0) shadow_ingest(idx, 0, idx->n, idx->n, nullptr, true);
  return SVS_OK;
}

int32_t svs_internal_ahead_stats(svs_index* idx, int64_t* out, int32_t cap) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(idx->mu);
  // shared passes: the claim kernels' counters, read from their pinned mirrors without synchronising
  int64_t shared = 0, claimed = 0, empty = 0, thin = 0, thin_worked = 0;
  for (const AheadPipe* p : idx->pipes) {
    const volatile uint32_t* h = p->share_mirror();
    empty += h[0];
    thin += h[SHARE_MAX + 1];
    thin_worked += h[SHARE_MAX + 2];
    for (int c = 2; c <= SHARE_MAX; ++c) {
      shared += h[c];
      claimed += (int64_t)(c - 1) * h[c];
    }
  }
  int64_t thin_grid = 0;
  if (cap > 12 && hipSetDevice(idx->device) == hipSuccess) thin_grid = thin_grid_of(idx);
  const int64_t v[13] = {idx->ahead_calls.load(), idx->ahead_plain.load(), idx->ahead_retired.load(), (int64_t)idx->pipes.size(),
                         idx->ahead_bound.load(), idx->ahead_records.load(), idx->ahead_waits.load(), shared, claimed, empty,
                         thin, thin_worked, thin_grid};
  for (int i = 0; i < cap && i < 13; ++i) out[i] = v[i];
  return SVS_OK;
}

// ---- test hooks: the selection stage alone on caller-given data (internal.h) -------------------
// The index supplies the device, a context and (candidates hook) its tombstone bitmap; the data and n are the
// caller's.  Each runs on the context's own stream and has drained it when it returns.
namespace {
constexpr int64_t HOOK_MAX_N = (int64_t)1 << 26;   // rows / k a hook accepts (the kernels themselves go to 2^32 rows)

// Non-zero words among the first nq * SCR_WORDS words of the context's select scratch, read back behind everything
// enqueued by the call (also waits for it).  A context whose scratch holds fewer than nq queries was not touched: 0.
int scratch_dirty(HostCall& fr, int nq, int64_t* out) {
  *out = 0;
  Ctx* const c = fr.c;
  std::vector<uint32_t> w;
  if ((size_t)nq <= c->hist_cap) {
    w.resize((size_t)nq * SCR_WORDS);
    HIP_TRY(hipMemcpyAsync(w.data(), c->hist, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, fr.stream()));
  }
  if (const int rc = fr.wait(); rc != SVS_OK) return rc;
  int64_t d = 0;
  for (uint32_t x : w) d += x != 0u;
  *out = d;
  return SVS_OK;
}
}  // namespace

int32_t svs_internal_select_scores(svs_index* idx, const float* scores, int32_t nq, int64_t n, int32_t k, int64_t row_offset,
                                   float* out_scores, int64_t* out_rows, int32_t* out_count, int64_t* out_dirty) {
  if (!idx || !scores || !out_scores || !out_rows || !out_count || !out_dirty) return fail(SVS_ERR_INVALID, "null argument");
  if (nq < 1 || nq > 1024 || n < 1 || n > HOOK_MAX_N || k < 1 || k > HOOK_MAX_N)
    return fail(SVS_ERR_INVALID, "svs_internal_select_scores: nq %d, n %lld, k %d out of range", nq, (long long)n, k);
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  const int count = (int)std::min<int64_t>(k, n);
  *out_count = count;
  const int64_t sstride = score_stride(n);   // float4-aligned score vectors, as plan_search lays them out
  const bool path_a = select_path(n, count) == SelectPath::WINDOW;
  HostCall fr(idx);
  int rc;
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  if ((rc = c->scores.grow((size_t)nq * (size_t)sstride)) != SVS_OK) return rc;
  if (path_a && (rc = grow_select_scratch(c, nq, st)) != SVS_OK) return rc;
  DevTmp tmp;
  float* d_s = nullptr;
  int64_t* d_r = nullptr;
  HIP_TRY(tmp.alloc(&d_s, (size_t)nq * k * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_r, (size_t)nq * k * sizeof(int64_t)));
  HIP_TRY(hipMemcpy2DAsync(c->scores, (size_t)sstride * sizeof(float), scores, (size_t)n * sizeof(float), (size_t)n * sizeof(float),
                           (size_t)nq, hipMemcpyHostToDevice, st));
  if ((rc = run_select(idx, c, c->scores, n, sstride, nq, k, count, d_s, d_r, st, row_offset)) != SVS_OK) return rc;
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(out_rows, d_r, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  return scratch_dirty(fr, nq, out_dirty);
}

int32_t svs_internal_kth_value(svs_index* idx, const float* scores, int32_t nq, int64_t n, int32_t k, int32_t misalign,
                               float* out_thr, int64_t* out_dirty) {
  if (!idx || !scores || !out_thr || !out_dirty) return fail(SVS_ERR_INVALID, "null argument");
  if (nq < 1 || nq > 1024 || n < 1 || n > HOOK_MAX_N || k < 1 || k > n)
    return fail(SVS_ERR_INVALID, "svs_internal_kth_value: nq %d, n %lld, k %d out of range (1 <= k <= n)", nq, (long long)n, k);
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  const int64_t sstride = score_stride(n);
  HostCall fr(idx);
  int rc;
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  if ((rc = c->scores.grow((size_t)nq * (size_t)sstride + 4)) != SVS_OK) return rc;
  if ((rc = c->pref_s.grow((size_t)nq)) != SVS_OK) return rc;
  float* base = c->scores.p + (misalign ? 1 : 0);   // one float off a 16-byte boundary: the kernel's streaming branch
  HIP_TRY(hipMemcpy2DAsync(base, (size_t)sstride * sizeof(float), scores, (size_t)n * sizeof(float), (size_t)n * sizeof(float),
                           (size_t)nq, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->pref_s, 0xff, (size_t)nq * sizeof(float), st));   // (a threshold nobody wrote reads back as NaN)
  hipLaunchKernelGGL(prefix_kth_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, (const float*)base, n, sstride, k, c->pref_s.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_thr, c->pref_s, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, st));
  return scratch_dirty(fr, nq, out_dirty);
}

int32_t svs_internal_select_candidates(svs_index* idx, const uint64_t* keys, const int64_t* key_offsets, const uint32_t* n_cand,
                                       int32_t nq, int32_t k, int32_t count, int32_t use_dead, float* out_scores,
                                       int64_t* out_rows, int64_t* out_dirty) {
  if (!idx || !key_offsets || !n_cand || !out_scores || !out_rows || !out_dirty) return fail(SVS_ERR_INVALID, "null argument");
  // (count <= 256: plan_search's rule for the fused path, whose lists these are)
  if (nq < 1 || nq > 1024 || count < 1 || count > FINAL_THREADS || k < count || k > HOOK_MAX_N)
    return fail(SVS_ERR_INVALID, "svs_internal_select_candidates: nq %d, k %d, count %d out of range", nq, k, count);
  RefGuard guard(idx);
  std::shared_lock<std::shared_mutex> geo(idx->rw);
  if (use_dead && idx->dead_list.empty()) return fail(SVS_ERR_INVALID, "svs_internal_select_candidates: the index has no masked rows");
  for (int q = 0; q < nq; ++q) {
    const int64_t len = key_offsets[q + 1] - key_offsets[q];
    if (key_offsets[q] < 0 || len != (int64_t)std::min<uint32_t>(n_cand[q], (uint32_t)CAND_CAP) || (len > 0 && !keys))
      return fail(SVS_ERR_INVALID, "svs_internal_select_candidates: query %d gives %lld keys for a claim of %u", q, (long long)len, n_cand[q]);
    if (use_dead)   // the kernel looks every row up in the bitmap
      for (int64_t i = key_offsets[q]; i < key_offsets[q + 1]; ++i)
        if ((int64_t)(uint32_t)keys[i] >= idx->n)
          return fail(SVS_ERR_INVALID, "svs_internal_select_candidates: row %u outside the index", (uint32_t)keys[i]);
  }
  HostCall fr(idx);
  int rc;
  if ((rc = fr.open()) != SVS_OK) return rc;
  Ctx* const c = fr.c;
  const hipStream_t st = fr.stream();
  if ((rc = grow_select_scratch(c, nq, st)) != SVS_OK) return rc;
  DevTmp tmp;
  float* d_s = nullptr;
  int64_t* d_r = nullptr;
  HIP_TRY(tmp.alloc(&d_s, (size_t)nq * k * sizeof(float)));
  HIP_TRY(tmp.alloc(&d_r, (size_t)nq * k * sizeof(int64_t)));
  // what the fused epilogue leaves: the keys in the order given, and a header that carries the claim
  std::vector<SelHeader> hdr((size_t)nq);
  auto run = [&]() -> int {
    for (int q = 0; q < nq; ++q) {
      hdr[q] = SelHeader{n_cand[q], 0u, 0u, 0u};
      const int64_t len = key_offsets[q + 1] - key_offsets[q];
      if (len > 0)
        HIP_TRY(hipMemcpyAsync(c->cand.p + (size_t)q * CAND_CAP, keys + key_offsets[q], (size_t)len * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(c->hist.p + (size_t)q * SCR_WORDS, &hdr[q], sizeof(SelHeader), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(select_final_kernel, dim3(nq), dim3(FINAL_THREADS), 0, st, (const float*)nullptr, idx->n, (int64_t)0, k, count, 3,
                       c->hist.p, c->cand.p, idx->row_offset, d_s, d_r, (const uint32_t*)(use_dead ? idx->dead_bits_dev.p : nullptr));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_scores, d_s, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_rows, d_r, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return scratch_dirty(fr, nq, out_dirty);
  };
  rc = run();
  if (rc != SVS_OK) {
    // A failed hook must not hand the context back with the headers it uploaded: the next search on it relies on an
    // all-zero scratch.  (Best effort, behind whatever is still queued and drained by the frame; the first error stays
    // the one reported.)
    (void)hipMemset2DAsync(c->hist.p, (size_t)SCR_WORDS * sizeof(uint32_t), 0, sizeof(SelHeader), (size_t)nq, fr.stream());
  }
  return rc;
}

int32_t svs_internal_screen_stats(svs_index* idx, int64_t* out, int32_t cap) {
  if (!idx || !out) return fail(SVS_ERR_INVALID, "null argument");
  int64_t v[9] = {};
  if (idx->scr_host) {
    const volatile uint32_t* h = idx->scr_host;
    for (int i = 0; i < svs_index::kSlots; ++i) {
      v[0] += h[i * SCREEN_SLOT_WORDS];
      v[1] += h[i * SCREEN_SLOT_WORDS + 1];
    }
    if (g_screen_idx == idx) {
      v[4] = h[g_screen_slot * SCREEN_SLOT_WORDS + 2];
      v[5] = h[g_screen_slot * SCREEN_SLOT_WORDS + 3];
    }
  }
  v[2] = idx->shadow_bad.load() ? 2 : (idx->shadow ? 1 : 0);
  v[3] = idx->scr_paused.load() ? 1 : 0;
  if (idx->scr_dev && idx->shadow) {
    HIP_TRY(hipSetDevice(idx->device));
    ScreenStats h{};
    HIP_TRY(hipMemcpy(&h, idx->scr_dev, sizeof h, hipMemcpyDeviceToHost));
    v[6] = h.A; v[7] = h.B; v[8] = h.C;
  }
  for (int i = 0; i < cap && i < 9; ++i) out[i] = v[i];
  return SVS_OK;
}

int32_t svs_index_set_variant(svs_index* idx, int32_t variant) {
  if (!idx) return fail(SVS_ERR_INVALID, "null index");
  if (variant < VARIANT_DEFAULT || variant > VARIANT_LAST) return fail(SVS_ERR_INVALID, "unknown variant %d", variant);
  idx->variant.store(variant);
  return SVS_OK;
}

}  // extern "C"

/*
 * internal.h -- entry points libsvs_amd.so exports for its OWN tests, tools and bench; NOT part of the
 * drop-in boundary (include/svs_amd.h) and not a contract: they may change or go in any round.
 */
#ifndef SVS_AMD_INTERNAL_H
#define SVS_AMD_INTERNAL_H
#include "../../include/svs_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The NEXT coalesced pass on this handle waits (at most 5 s) until n single-query calls are queued, so that a
 * pass of a chosen size can be formed on purpose (parity tests of the coalesced route); one shot, 0 cancels. */
int32_t svs_internal_coalesce_hold(svs_index* idx, int32_t n);
/* Process-wide knobs for A/B measurements:
 *   0  fused path: threshold prefix = n / value rows (default 64; at least 16,384 rows)
 *   1  host batches: 0 = f16 batches pulled from pinned memory by the staging kernel, chunk by chunk (default);
 *      1 = staged DMA for every dtype (round 3)
 *   2  fused path's threshold rows: 1 = a sample spread over the whole corpus (default); 0 = the first rows (rounds 1-3)
 *   3  1 = every allocation of an f32 index's half shadow is refused, as if HBM were full (default 0)
 *   4  run-ahead pipelines MADE FROM NOW ON: 0 = a pass's last kernel carries its completion event and the pass stream
 *      waits for a selection once per group of passes (default); 1 = an event record behind every pass and a wait in
 *      front of every pass
 *   5  run-ahead pipelines MADE FROM NOW ON: queries one score pass may serve (1 .. SHARE_MAX; 1 = no shared passes)
 *   6  run-ahead pipelines, the grid of a shareable search's own pass: 0 = thin (one resident set of workgroups) where the
 *      host predicts that an earlier pass serves the search (default); 1 = always the one-shot grid; 2 = always thin
 *   7  svs_index_search_by_label, what crosses workgroups (by_label.h): 0 = integer atomics on the query's table in HBM
 *      (default); 1 = one partial table per workgroup, reduced by the final kernel.  The same bits either way.
 *   8  svs_index_search_combined, the route (combine.h): 0 = the route's own choice (default); 1 = the fused kernel
 *      wherever the row length has one; 2 = always m single-query passes and combine_scores_kernel.  The same bits. */
int32_t svs_internal_tune(int32_t what, int64_t value);
/* Seconds since the start of the calling thread's last svs_index_search(host batch) at which: [0] scratch was planned,
 * [1] the queries were in pinned memory (and their DMA enqueued), [2] every kernel was enqueued, [3] the stream had
 * drained, [4] the results were in the caller's buffers; [5] = the number of the call's queries whose fused candidate list
 * overflowed and that were re-run through the materialised path (a count, not a time). */
int32_t svs_internal_host_phases(double* out, int32_t n);
/* The score kernels the calling thread's last svs_index_search, svs_index_search_device or svs_index_scores_n call
 * enqueued, in order (each of those calls starts a new record): kernels[i] is the kernel with its template arguments as
 * c++filt prints it, without the svs:: of the function ("gemm_phased_kernel<true, 2, 20, 256>",
 * "gemv_unrolled_kernel<64, 2, 4, svs::DotF16>"; a static string).  The single-query kernels are announced by one "gemv"
 * entry for the whole per-query loop (nq = the loop's queries), followed by one entry per query with the kernel that
 * query's launch_scores enqueued (nq = 1); a screened search lists its gemv_f16_oneshot_kernel and rescore_f32_kernel
 * without a "gemv" entry.  rows[i] is the entry's row count (a fused search's threshold pass covers fewer rows than
 * the corpus); nq[i] its query count.  A fused search whose candidate lists overflowed lists the materialised re-run's
 * launches after its own.  Up to cap entries (and at most 64) are written; returns the number of launches recorded.
 * Coalesced single-query passes and svs_multi_* launch from other threads: they are not in the caller's record. */
int32_t svs_internal_last_launches(const char** kernels, int64_t* rows, int32_t* nq, int32_t cap);
/* The kernel a single query takes on an index of dtype and dimension d under svs_index_set_variant(variant), screened
 * (screen != 0: an f32 index that has a half shadow) or not: pure host code, no index and no device.  kernel[cap] gets
 * the name as svs_internal_last_launches spells it, from the dispatch that launches it; *flags: bit 0 = the pass can serve
 * other searches of a run-ahead pipeline, bit 1 = the kernel reads ld query floats, so the query is copied (zero padded)
 * when the rows are padded beyond d. */
int32_t svs_internal_single_route(int32_t dtype, int32_t d, int32_t variant, int32_t screen, char* kernel, int32_t cap, int32_t* flags);
/* The kernel one pass of a batch of nq >= 2 queries takes on an index of dtype and dimension d under
 * svs_index_set_variant(variant): pure host code, no index and no device, through the dispatch that launches (batch_route,
 * launch_batch in its name-only mode).  n_rows >= 1: the rows the pass covers (a fused search's threshold pass covers
 * fewer than the corpus); flags: bit 0 = the fused epilogue, bit 1 = pair mode (svs_index_top_pairs).  kernel[cap] gets the
 * name as svs_internal_last_launches spells it, "gemv" for the per-query loop of the single-query kernels.  info[3], what
 * the call decides once for all its passes: [0] family (0 per-query loop, 1 the 16-query kernels, 2 the f32 tiled kernel,
 * 3 the f16 / fp8 tiled and phased kernels), [1] queries per group or query tile (1 for the loop), [2] rows of the staged
 * query image (nq rounded up to [1]).  SVS_ERR_INVALID for what no index has (dtype, d < 1, variant, nq < 2) and for pair
 * mode on the 16-query family, which has none. */
int32_t svs_internal_batch_route(int32_t dtype, int32_t d, int32_t variant, int32_t nq, int64_t n_rows,
                                 int32_t flags /* bit 0 fused, bit 1 pair mode */, char* kernel, int32_t cap,
                                 int32_t* info /* [0] family, [1] queries per tile, [2] staged rows */);
/* The groups in which the host re-runs the overflowed positions of [q0, q1) of a result block, pure host code: res_rows =
 * the block's rows at stride count (a position is marked by -2 in its first entry), max = positions per group
 * (1 .. 256; a search derives it from the index's row count).  positions[q1 - q0] gets the marked positions, group after
 * group; sizes[q1 - q0] each group's size, *n_groups their number.  Returns the number of marked positions, or
 * SVS_ERR_INVALID. */
int64_t svs_internal_redo_groups(const int64_t* res_rows, int32_t count, int64_t q0, int64_t q1, int32_t max, int64_t* positions,
                                 int64_t* sizes, int64_t* n_groups);
/* Screened search (screen.h) on this handle, up to cap (<= 9) values: [0] queries answered from the candidate list,
 * [1] queries that took the exact whole-corpus fallback (both as the kernels last wrote them to pinned memory: drain
 * the stream first), [2] shadow: 0 none, 1 valid, 2 invalid for good (an element half cannot hold), [3] 1 = screening
 * paused until the next ingest (fallbacks dominated), [4] bits of the bound E and [5] candidate count of the calling
 * thread's last screened search, [6..8] bits of the corpus statistics A, B, C. */
int32_t svs_internal_screen_stats(svs_index* idx, int64_t* out, int32_t cap);
/* svs_index_search_device_ahead on this handle, up to cap (<= 13) values: [0] single-query calls that went through a
 * pipeline, [1] single-query calls that were plain calls because every pipeline had work in flight, [2] idle
 * pipelines handed over to another caller stream, [3] pipelines that exist, [4] passes whose completion event was
 * carried by their last kernel, [5] event records enqueued on pass streams (the timing events among them), [6] waits
 * enqueued on pass streams, the caller's query_ready_event not counted; then the shared passes' counters as the claim
 * kernels last wrote them to pinned memory (drain the stream first): [7] passes that served more than one search,
 * [8] searches served by an earlier search's pass, [9] passes that found their search served; [10] passes launched on
 * a thin grid, [11] those among them that had work after all, [12] workgroups of the thin grid for this index's row
 * length (0: its passes are never shared). */
int32_t svs_internal_ahead_stats(svs_index* idx, int64_t* out, int32_t cap);
/* The top-k stage ALONE on caller-given data (tests/test_select_routes_gpu.py).  The index supplies the device, a search
 * context and, where asked, its tombstone bitmap; n is the caller's, not the index's.  Each hook runs on the context's own
 * stream, has drained it when it returns, and reports in *out_dirty the number of non-zero words among the nq per-query
 * scratch blocks (header + window histogram) of that context, read back behind the selection: the stage's invariant is 0.
 *
 * svs_internal_select_scores: run_select over host scores[nq][n] (copied to float4-aligned device rows), scratch grown as
 *   a search grows it.  out_scores / out_rows are [nq][k], filled past *out_count = min(k, n) with -inf / -1. */
int32_t svs_internal_select_scores(svs_index* idx, const float* scores, int32_t nq, int64_t n, int32_t k, int64_t row_offset,
                                   float* out_scores, int64_t* out_rows, int32_t* out_count, int64_t* out_dirty);
/* svs_internal_kth_value: prefix_kth_kernel over host scores[nq][n], 1 <= k <= n; out_thr[nq].  misalign != 0 places the
 *   device rows one float off a 16-byte boundary, so that the kernel takes its streaming branch whatever n. */
int32_t svs_internal_kth_value(svs_index* idx, const float* scores, int32_t nq, int64_t n, int32_t k, int32_t misalign,
                               float* out_thr, int64_t* out_dirty);
/* svs_internal_select_candidates: select_final_kernel on candidate lists as the fused epilogue leaves them.  Query q's
 *   keys (score key << 32 | local row, unique rows) are keys[key_offsets[q] .. key_offsets[q + 1]), uploaded in the order
 *   given; its header claims n_cand[q] candidates, and exactly min(n_cand[q], 32768) keys must be given.  1 <= count <= 256,
 *   count <= k.  use_dead != 0 strikes out the index's masked rows (every row must then lie inside the index).  out_scores /
 *   out_rows are [nq][k]; a query the kernel could not answer has -2 in every out_rows entry. */
int32_t svs_internal_select_candidates(svs_index* idx, const uint64_t* keys, const int64_t* key_offsets, const uint32_t* n_cand,
                                       int32_t nq, int32_t k, int32_t count, int32_t use_dead, float* out_scores,
                                       int64_t* out_rows, int64_t* out_dirty);
/* The steps of an in-place compaction (compact.h), pure host code: dead_sorted = the ndead tombstoned local rows of an
 * n-row index, strictly ascending.  steps[3 i ..] = kind (0 DIRECT: one launch, dst0 + count <= source of dst0; 1 BOUNCE:
 * through the bounce buffer, count <= bounce_rows), dst0, count; ascending and contiguous from the first dead row to
 * n - ndead.  Up to cap steps are written; returns the number of steps of the plan, or SVS_ERR_INVALID. */
int64_t svs_internal_compact_plan(const uint32_t* dead_sorted, int64_t ndead, int64_t n, int64_t bounce_rows, int64_t* steps, int64_t cap);
/* svs_index_compact with a bounce buffer of bounce_rows rows (<= 0: the default).  stats[4] (may be NULL): DIRECT steps,
 * BOUNCE steps, rows moved, bytes moved (rows, scales and shadow rows, each byte counted once). */
int32_t svs_internal_compact(svs_index* idx, int64_t bounce_rows, int64_t* out_old_rows, int64_t cap, int64_t* out_n, int64_t* stats);
/* The tile table of svs_index_search_segments (segments.h), pure host code, no index: sizes[nseg] = live rows per
 * segment, seg_query[nseg] or NULL (segment s takes query s), w = rows a wave of the score kernel takes.  Segments of
 * 1 .. 4096 rows get ceil(size / w) tiles at consecutive list offsets in segment order, the others none.
 * tiles[4 i ..] = list (and score) offset, rows in the tile (1 .. w), query, segment; up to cap tiles are written.
 * seg_off[nseg] (may be NULL): a tiled segment's list offset, -1 for the others; *total_rows (may be NULL): the rows
 * the tiles cover.  Returns the number of tiles of the plan, SVS_ERR_UNSUPPORTED when they cover 2^31 rows or more,
 * or SVS_ERR_INVALID. */
int64_t svs_internal_segments_plan(const int64_t* sizes, const int32_t* seg_query, int64_t nseg, int32_t w, int64_t* tiles, int64_t cap,
                                   int64_t* seg_off, int64_t* total_rows);
/* The device row list of svs_index_search_rows and of every segment of svs_index_search_segments, pure host code, no
 * index: rows[nrows] = global rows in any order, repeats allowed, every one in [row_offset, row_offset + n);
 * dead_flags[n] = non-zero for a tombstoned local row.  out[0 .. m) gets the distinct live listed rows as local rows,
 * ascending; cap = the room in out, at least nrows.  Returns m, or SVS_ERR_INVALID with out untouched. */
int64_t svs_internal_live_rows(const int64_t* rows, int64_t nrows, int64_t row_offset, int64_t n, const uint8_t* dead_flags, uint32_t* out,
                               int64_t cap);
/* Rows per workgroup strip of the label filter (labels.h, LB_STRIP): the sizes at which svs_index_search_labeled's
 * kernels change what they do (tests). */
int32_t svs_internal_labels_strip(void);
/* svs_index_search_by_label's reduce kernel (by_label.h): out[0] = rows per strip (BL_STRIP), out[1] = the most
 * workgroups of a launch (BL_GRID_MAX); an index of more than out[0] * out[1] rows gives a workgroup several strips
 * (tests). */
int32_t svs_internal_by_label_geometry(int32_t* out);
/* svs_index_search_collapsed's reduce and mark kernels (collapse.h): out[0] = rows per strip (CL_STRIP), out[1] = the
 * most workgroups of a launch (CL_GRID_MAX); an index of more than out[0] * out[1] rows gives a workgroup several
 * strips (tests). */
int32_t svs_internal_collapse_geometry(int32_t* out);
/* Milliseconds between the HIP events around the stages of the LAST query of the calling thread's last
 * svs_index_search_collapsed, recorded while svs_index_set_timing is on for the handle: out[0] collapse_reduce_kernel,
 * out[1] collapse_mark_kernel, out[2] the table's fill, out[3] the top-k stage; -1 where that call recorded none
 * (tools/collapse_time.py). */
int32_t svs_internal_collapse_kernel_ms(double* out);
/* Milliseconds between the HIP events around the stages of the calling thread's last svs_index_search_collapsed_where
 * or svs_index_search_collapsed_rows, recorded while svs_index_set_timing is on for the handle: out[0] the filter (the
 * counting launch plus the scan and scoped_write_kernel; _rows: the list's upload and scoped_values_kernel), out[1]
 * the last query chunk's gather launch, and for the LAST query out[2] collapse_reduce_kernel, out[3]
 * collapse_mark_kernel, out[4] the table's fill, out[5] the top-k stage; -1 where that call recorded none
 * (tools/collapse_where_time.py). */
int32_t svs_internal_collapse_scope_kernel_ms(double* out);
/* Milliseconds between the HIP events around assign_rows_kernel in the calling thread's last svs_index_assign, recorded
 * while svs_index_set_timing is on for the handle; -1 when that call recorded none (tools/assign_time.py). */
int32_t svs_internal_assign_kernel_ms(double* out);
/* Milliseconds between the HIP events around label_sums_chunk_kernel and label_sums_fold_kernel in the calling thread's
 * last svs_index_label_sums, recorded while svs_index_set_timing is on for the handle; -1 when that call recorded none
 * (a count-only call, tools/label_sums_time.py). */
int32_t svs_internal_label_sums_kernel_ms(double* out);
/* The unmasked combined score vector of ONE combined query (svs_index_search_combined: m vectors [m][d], weights [m] or
 * NULL, op) over all n local rows, into out[0 .. n) (capacity >= n floats).  route: 0 = the route's choice, 1 = the
 * fused kernel (SVS_ERR_UNSUPPORTED where the row length has none), 2 = m passes and combine_scores_kernel (tests). */
int32_t svs_internal_combined_scores(svs_index* idx, const float* vectors, int32_t m, int32_t d, const float* weights, int32_t op,
                                     int32_t route, float* out, int64_t capacity);
/* The m unmasked score vectors of ONE combined query (m vectors [m][d]) over all n local rows, vector j into
 * out[j * n .. (j + 1) * n) (capacity >= m * n floats): what svs_index_search_collapsed_combined's group stage reads.
 * route: 0 = the route's choice, 1 = the fused multi-score kernel (SVS_ERR_UNSUPPORTED where the row length has none),
 * 2 = m single-query passes (tests).  Every route gives the bits of svs_index_scores_n per vector. */
int32_t svs_internal_multi_scores(svs_index* idx, const float* vectors, int32_t m, int32_t d, int32_t route, float* out, int64_t capacity);
/* Milliseconds between the HIP events around the score pass (the fused kernel, or the m passes and what follows them) in
 * the calling thread's last svs_internal_combined_scores or svs_internal_multi_scores, recorded while
 * svs_index_set_timing is on for the handle; -1 when that call recorded none (tools/collapsed_combined_time.py: the
 * multi-score kernel against the combine kernel of the same shape and m). */
int32_t svs_internal_score_pass_ms(double* out);
/* Milliseconds between the HIP events around the stages of the LAST query of the calling thread's last
 * svs_index_search_collapsed_combined, recorded while svs_index_set_timing is on for the handle: out[0] the score
 * pass(es), out[1] cc_reduce_kernel, out[2] cc_mark_kernel, out[3] the fills of the table and the keys, out[4] the top-k
 * stage; -1 where that call recorded none (tools/collapsed_combined_time.py).  The kernels share the geometry
 * svs_internal_collapse_geometry reports. */
int32_t svs_internal_collapsed_combined_kernel_ms(double* out);
/* What ingest left in HBM, byte for byte (tests/test_ingest_image_gpu.py): plain device-to-host copies behind
 * staging_wait and under the shared geometry lock, no kernel, nothing left on a stream.  Rows [row0, row0 + nrows) of
 *   what 0  the corpus rows: nrows * ld * element bytes, the padding columns from d to ld included;
 *   what 1  the fp8 row scales: nrows floats;
 *   what 2  the half shadow of an f32 index: nrows * ld * 2 bytes.
 * SVS_ERR_UNSUPPORTED when the index has no such image (scales of an f32 / f16 index, no shadow); SVS_ERR_INVALID for a
 * null index or out, an unknown what, a range outside [0, n) or a capacity_bytes smaller than the image. */
int32_t svs_internal_stored_image(svs_index* idx, int32_t what, int64_t row0, int64_t nrows, void* out, int64_t capacity_bytes);
/* multi.hip -> svs_amd.hip: carries a worker thread's error message over to the caller's thread */
int32_t svs_internal_set_error(int32_t code, const char* msg);
#ifdef __cplusplus
}
#endif
#endif

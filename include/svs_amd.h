/*
 * svs_amd.h -- C ABI of the MI355X (gfx950) brute-force similarity backend for SVS.
 *
 * This is the drop-in boundary for the ONE hot path of Rhobota/svs v0.7.4: the
 * cosine-similarity + top-k search inside KB.retrieve()/AsyncKB.retrieve().
 * The reference has no FFI of its own (it is pure Python + NumPy), so each entry
 * point below cites the reference lines it replaces; INTEGRATION.md shows the
 * ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions / abort() cross this boundary;
 *   - every function returns SVS_OK (0) or a negative svs_status; the message for
 *     the calling thread's last failure is svs_last_error() (thread-local);
 *   - status -> Python exception the host wrapper raises, matching the reference:
 *       SVS_ERR_SHAPE   ValueError  (numpy: "shapes (N,D) and (d,) not aligned",
 *                                    src/svs/kb.py:1623 with a wrong-sized query)
 *       SVS_ERR_INVALID ValueError  (bad argument)
 *       SVS_ERR_DEVICE  RuntimeError (HIP failure)     SVS_ERR_NOMEM MemoryError
 *   - an index handle is reference counted: create() returns it with one
 *     reference; search calls hold a reference for their duration, so release()
 *     from _EmbeddingsMatrix.invalidate() (src/svs/kb.py:861-864) may race with
 *     an in-flight AsyncKB search on an executor thread (src/svs/kb.py:1184-1190);
 *   - all search entry points are re-entrant on one handle.
 */
#ifndef SVS_AMD_H
#define SVS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svs_index svs_index;

typedef enum svs_status {
  SVS_OK = 0,
  SVS_ERR_INVALID = -1,
  SVS_ERR_SHAPE = -2,
  SVS_ERR_DEVICE = -3,
  SVS_ERR_NOMEM = -4,
  SVS_ERR_UNSUPPORTED = -5
} svs_status;

/* element type of the HBM-resident corpus (the arithmetic stays f32-accumulate) */
typedef enum svs_dtype {
  SVS_DTYPE_F32 = 0, /* reference layout: np.zeros((n, m), float32), src/svs/kb.py:600 */
  SVS_DTYPE_F16 = 1, /* extension for BASELINE.json configs[2]/[3]: rows AND queries rounded to IEEE
                        half (RNE), products exact in f32, f32 accumulate.  Parity oracle: numpy's
                        f32 path on the dequantised corpus and query. */
  SVS_DTYPE_FP8 = 2  /* extension for BASELINE.json configs[4]: OCP e4m3fn rows with one f32 scale per
                        row (max|x| -> 448), queries quantised the same way; score = scale_row *
                        scale_query * sum(q8 * q8) accumulated in f32.  Same oracle rule.
                        scale = max(max|x|, 7 * 2^-120) / 448 (NaN elements skipped; 1 for an all-zero
                        row), q8 = e4m3(x * (1 / scale)), round to nearest even.  The floor keeps the scale at
                        or above 2^-126 so that every finite row reads back finite and zeros read back as zeros
                        (|stored - x| <= 17 * max(max|x|, 7 * 2^-120) / 448); elements of a row below the floor
                        quantise against the floor, possibly to zero.  A NaN element is stored as NaN and does
                        not touch its row's scale.  A row, or query, with an INFINITE element gets scale inf:
                        every element of it reads back as NaN, and NaN ranks first.  (Batches of more
                        than 16 queries run on the fp8 matrix instruction, whose internal sum of 128 products
                        keeps ~13 bits below the largest one: scores within 3e-6 of the exact dot product of the
                        quantised values on unit-norm data, up to 1.4e-4 relative when a single product
                        dominates; single queries use f32 FMAs: 2e-7.) */
} svs_dtype;

typedef struct svs_index_info_t {
  int64_t n;          /* rows held by this handle (one shard)                 */
  int32_t d;          /* logical dimension                                     */
  int32_t ld;         /* padded row stride in elements (HBM layout)            */
  int32_t dtype;      /* svs_dtype                                             */
  int32_t device;     /* HIP device ordinal                                    */
  int64_t row_offset; /* global row index of local row 0 (row sharding, 8(e))  */
  int64_t hbm_bytes;  /* bytes of HBM held by the corpus (an f32 index's half shadow included: svs_index_set_screen) */
  int64_t n_masked;   /* rows tombstoned by svs_index_mask_rows (still counted in n) */
} svs_index_info_t;

/* Stages timed with HIP events on the stream the kernels run on (bench.py roofline). */
typedef struct svs_timing_t {
  double score_ms_sum;  /* dominant kernel: query x corpus GEMV/GEMM            */
  double select_ms_sum; /* top-k select + order kernels                          */
  int64_t launches;     /* number of searches accumulated                        */
  double dominant_ms_sum; /* the ONE dominant kernel launch inside the score stage: for a fused batched
                             search the whole-corpus GEMM (without query staging and the prefix pass that
                             seeds its thresholds); otherwise equal to score_ms_sum              */
} svs_timing_t;

/* ---- library ------------------------------------------------------------- */
const char* svs_version(void);
const char* svs_last_error(void);
/* Number of visible HIP devices (0 when none; never fails). */
int32_t svs_device_count(void);
/* Free / total HBM of a device in bytes (capacity planning, leak tests). */
int32_t svs_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes);

/* ---- index lifetime: replaces the cached (embeddings_matrix, emb_id_lookup)
 *      pair of _EmbeddingsMatrix, src/svs/kb.py:856-893 --------------------- */

/* One pinned-staged H2D copy of a C-contiguous f32 (n, d) host matrix -- the
 * array _Querier.build_embeddings_matrix returns (src/svs/kb.py:573-618) -- into
 * HBM on `device`.  The library copies, never aliases: the caller keeps owning
 * host_rows.  n == 0 or d == 0 is representable (search then reports
 * SVS_ERR_SHAPE, like numpy on a (0,0) matrix).  row_offset is added to every
 * returned row index (row-sharded corpora; 0 for a whole corpus). */
int32_t svs_index_create(const float* host_rows, int64_t n, int32_t d, int32_t store_dtype,
                         int32_t device, int64_t row_offset, svs_index** out);

/* Same, from rows already in device memory on `device` (f32, row stride
 * src_ld elements): synthetic corpora generated on the GPU, shards staged
 * GPU->GPU.  Copies; does not alias. */
int32_t svs_index_create_from_device(const float* dev_rows, int64_t n, int32_t d, int64_t src_ld,
                                     int32_t store_dtype, int32_t device, int64_t row_offset,
                                     svs_index** out);

/* ---- incremental update: instead of dropping the whole cached matrix on every
 *      bulk_add_docs / bulk_del_docs (invalidate(), src/svs/kb.py:1523, :1541, :1062, :1086)
 *      and re-uploading 6-300 GB, the HBM copy is edited in place. */

/* Appends n_new rows (f32, C-contiguous (n_new, d), host) behind the existing ones:
 * new local rows n .. n+n_new-1, exactly where `SELECT id, embedding FROM embeddings`
 * (src/svs/kb.py:603-609) puts newly inserted embeddings.  Grows the HBM buffers by
 * 1.5x when needed.  Blocks searches on this handle while it runs. */
int32_t svs_index_append(svs_index* idx, const float* host_rows, int64_t n_new);

/* Same, from rows already in device memory on the index's device (f32, row stride src_ld
 * elements): corpora generated or staged on the GPU block by block, so that the f32 source of a
 * 10M x 3072 fp8 corpus (123 GB) never has to exist at once.  With svs_index_create(NULL, 0, d, ...)
 * + svs_index_reserve() this builds an index of any size from device blocks without a
 * reallocation.  Copies; does not alias. */
int32_t svs_index_append_from_device(svs_index* idx, const float* dev_rows, int64_t n_new, int64_t src_ld);

/* Grows the HBM buffers to hold rows_capacity rows (no-op when they already do), so that the
 * appends that follow neither reallocate nor copy.  The matrix the reference builds is sized
 * from SELECT COUNT(*) up front the same way (src/svs/kb.py:574-601). */
int32_t svs_index_reserve(svs_index* idx, int64_t rows_capacity);

/* ---- cold start without a host matrix: replaces the row loop of _Querier.build_embeddings_matrix,
 *      src/svs/kb.py:603-615 (98.7 s per 1M rows published) ---------------
 * The caller decodes SQLite BLOBs (little-endian f32, src/svs/embeddings/util.py:15-23) STRAIGHT
 * into pinned staging memory owned by the library and commits block after block; the DMA of block i
 * overlaps the filling of block i + 1 (two 32 MiB blocks).  No (n, m) host matrix, no second host
 * copy.  One producer at a time per handle; searches issued before svs_index_staging_finish() wait
 * for the pending copies first.
 *   acquire: a pinned block of *rows_cap rows x d floats the caller may fill (blocks until the DMA
 *            that last read this block has finished);
 *   commit:  appends the first n_rows rows of the block last acquired behind the existing rows
 *            (as svs_index_append) and returns once the copy is ENQUEUED;
 *   finish:  waits for every pending copy and frees the staging blocks. */
int32_t svs_index_staging_acquire(svs_index* idx, float** host_block, int64_t* rows_cap);
int32_t svs_index_staging_commit(svs_index* idx, int64_t n_rows);
int32_t svs_index_staging_finish(svs_index* idx);

/* Tombstones rows (GLOBAL indices, i.e. row_offset + local): they keep their index
 * (later rows do not shift, so the caller's emb_id_lookup stays valid) but can never
 * be returned again; count = min(k, n - masked).  Relative order of the surviving rows
 * is unchanged, so results equal those of a rebuilt matrix up to the row numbering. */
int32_t svs_index_mask_rows(svs_index* idx, const int64_t* rows, int64_t count);

/* Physically removes the tombstoned rows: live local row r becomes r - (dead rows below r); n shrinks by
 * n_masked, n_masked becomes 0.  Capacity and hbm_bytes are unchanged (the tail serves later appends).
 * out_old_rows[p] (p < new n) = the GLOBAL row that new local row p was; may be NULL.  If out_capacity <
 * live rows (and out_old_rows != NULL) nothing is done: SVS_ERR_INVALID, *out_n = live rows.  *out_n
 * (may be NULL) = rows after the call.  No tombstones: SVS_OK, nothing launched, identity map.
 *   - The rows move inside the HBM image (the relative order is kept, so the result is the matrix a rebuild from
 *     the live rows would hold); besides a bounce buffer of about 32 MiB, freed before the call returns, nothing
 *     is allocated.  Afterwards every entry point works as on an index freshly built from the live rows.
 *   - Like the ingest calls it holds a reference and the geometry lock exclusively: searches on this handle
 *     wait, and a search is never half-way through a compaction.  It waits for pending staging copies and for
 *     everything the device entries have enqueued before the first row moves.
 *   - RENUMBERING: a row index obtained before the call names another row (or none) after it.  Rows written by
 *     svs_index_search_device / _ahead searches enqueued BEFORE the call are in the old numbering, those of later
 *     searches in the new one; a caller that keeps a row -> id table applies out_old_rows to it.
 *   - Failures: a bad argument, a map that is too small and SVS_ERR_NOMEM (no HBM for a bounce buffer of even one
 *     row) leave the handle untouched.  SVS_ERR_DEVICE after the first move: the rows are in no defined order and
 *     the handle is only good for svs_index_release.
 *   - Not for the shards of an svs_multi (svs_multi_shard): the global numbering of svs_multi_search assumes the
 *     shard boundaries it was created with. */
int32_t svs_index_compact(svs_index* idx, int64_t* out_old_rows, int64_t out_capacity, int64_t* out_n);

int32_t svs_index_retain(svs_index* idx);
/* Drops one reference; HBM is freed when the last holder (including in-flight
 * searches) lets go.  Called from invalidate(), src/svs/kb.py:861-864. */
int32_t svs_index_release(svs_index* idx);
int32_t svs_index_info(const svs_index* idx, svs_index_info_t* out);

/* ---- search: replaces np.dot + get_top_k of superheavy(),
 *      src/svs/kb.py:1622-1627 (sync) / :1184-1189 (async),
 *      src/svs/util.py:190-203 ----------------------------------------------- */

/* nq queries (f32, C-contiguous (nq, d), host memory).  Per query:
 *   count = min(max(k, 0), n)            (src/svs/util.py:198-201)
 *   out_scores[i*k .. i*k+count)  f32 dot products, descending
 *   out_rows  [i*k .. i*k+count)  row_offset + local row; order is
 *                                 (score desc, row desc)  (src/svs/util.py:203)
 * Rows are ROW indices; the caller applies emb_id_lookup (src/svs/kb.py:1626).
 * d != index d -> SVS_ERR_SHAPE.  Blocks until the results are in the output
 * buffers.  The corpus is NOT re-normalised (vectors are validated unit-norm by
 * the reference, src/svs/embeddings/util.py:26-41, so cosine == dot). */
int32_t svs_index_search(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                         float* out_scores, int64_t* out_rows, int32_t* out_count);

/* Coalescing of concurrent single-query searches (off by default).  AsyncKB.retrieve runs its np.dot on
 * an executor thread outside the KB lock (src/svs/kb.py:1184-1190), so a server has many threads inside the
 * search at once; with enable != 0, svs_index_search calls with nq == 1 that arrive while the device is busy
 * are queued and answered TOGETHER by one batched pass over the corpus when it is free (up to 256; a call that
 * finds the device idle runs at once, alone).  The answer is the SAME total order (score desc, row desc,
 * src/svs/util.py:203) applied to scores that can differ from the single-query kernels' in the last bits
 * (the batched kernels sum in another order, far inside 1e-5): two rows whose scores are closer than that
 * rounding noise may therefore come out swapped, exactly as between two runs of numpy's own sgemv with
 * different blocking (hard part 1).  On every golden corpus recorded from the reference the
 * coalesced rows equal the reference's position by position (tests/test_search_gpu.py::test_search_golden).  Errors stay with the
 * call that made them.  svs_index_coalesce_stats: passes made / queries answered through this path;
 * svs_index_coalesce_sizes: out[s] = passes that carried exactly s queries, s < cap (cap <= 257). */
int32_t svs_index_set_coalesce(svs_index* idx, int32_t enable);
int32_t svs_index_coalesce_stats(svs_index* idx, int64_t* passes, int64_t* queries);
int32_t svs_index_coalesce_sizes(svs_index* idx, int64_t* out, int32_t cap);
/* Device-resident variant for pipelines and the multi-GPU gather (8(e)): queries
 * and outputs are device pointers on the index's device, work is enqueued on
 * `hip_stream` (a hipStream_t; NULL = the default stream) and the call returns
 * without synchronising.  Output layout as above with stride k; entries past
 * count are filled with score = -inf, row = -1.  *out_count is written on the
 * host immediately (it depends only on k and n). */
int32_t svs_index_search_device(svs_index* idx, const float* dev_queries, int32_t nq, int32_t d,
                                int32_t k, float* dev_out_scores, int64_t* dev_out_rows,
                                int32_t* out_count, void* hip_stream);

/* svs_index_search_device for back-to-back single queries: the score pass of one search runs beside the
 * selection kernels of the search before it.  Same arguments, outputs and results (rows, order, score bits).
 *   - Results are ordered on `hip_stream` exactly as with svs_index_search_device: work enqueued on that
 *     stream after the call sees them.
 *   - The SCORE stage runs on a stream of the library's own, one pass after another, and may start before
 *     earlier work on `hip_stream` has finished: the query is NOT ordered by that stream.  If
 *     `query_ready_event` (a hipEvent_t) is not NULL, the score stage runs once that event has fired; if it
 *     is NULL, the query must already be complete on the device when the call is made.
 *   - The query buffer may be reused by work ordered on `hip_stream` after the call (the stream waits for
 *     the score pass and for everything else that reads the query).
 *   - With nq != 1 the call is svs_index_search_device (behind query_ready_event, if given).
 *   - An index keeps at most four pipelines, one per caller stream.  A stream that has none when four exist takes
 *     over one whose work has all finished (least recently used first), so any number of streams may use the
 *     entry one after another.  Only while four OTHER streams each have such searches still in flight is the
 *     call an svs_index_search_device call: same results, no overlap.
 *   - Searches queued on one pipeline may be served by ONE pass over the corpus: a pass that starts while the
 *     searches behind it are already enqueued scores their queries from the rows it has loaded (up to four per
 *     pass).  Results are bit-identical to searches served one by one.  It relies on the rule above: a query
 *     without a ready event must be complete on the device when the call is made, because an EARLIER search's
 *     pass may read it.  A search with a ready event is always served by its own pass.
 * Ingest (append, reserve, staging commit, mask_rows, compact, set_screen) and svs_index_release may be called with
 * such searches enqueued, as with svs_index_search_device: they wait for what they would disturb. */
int32_t svs_index_search_device_ahead(svs_index* idx, const float* dev_query, int32_t nq, int32_t d, int32_t k,
                                      float* dev_out_scores, int64_t* dev_out_rows, int32_t* out_count,
                                      void* hip_stream, void* query_ready_event);

/* All scores of one query, f32 (n) to host: the raw `np.dot(M, q)` vector
 * (src/svs/kb.py:1623) for callers that want it and for parity tests.  The call writes one float per
 * row the handle holds WHEN IT RUNS and never more than out_capacity: a handle that has grown past the
 * caller's buffer (svs_index_append / svs_index_staging_commit from another thread between sizing the
 * buffer and this call) is SVS_ERR_INVALID, not an overflow -- the row count is read under the same
 * lock that appends take exclusively.  *out_n (may be NULL) = the rows the handle holds, written in
 * every case, so a caller can re-size and retry.  (Replaces round 3's svs_index_scores(idx, q, d, out),
 * which had no capacity and overflowed the caller's heap in exactly that race; the old symbol is gone
 * on purpose: a stale binding fails at load time instead of corrupting memory.) */
int32_t svs_index_scores_n(svs_index* idx, const float* query, int32_t d, float* out_scores,
                           int64_t out_capacity, int64_t* out_n);

/* Filtered search: svs_index_search over a caller-given subset of the rows (one book's chunks, one
 * user's files, one level of the document tree).  Generalises np.dot + get_top_k of superheavy()
 * (src/svs/kb.py:1622-1627, src/svs/util.py:190-203) to get_top_k(np.dot(M[S], q), k) with position
 * p mapped to S[p], where S = the live rows of `rows`, ascending, duplicates collapsed:
 *   rows      GLOBAL rows (row_offset + local, like svs_index_mask_rows), any order, duplicates
 *             allowed; a row outside [row_offset, row_offset + n) -> SVS_ERR_INVALID; tombstoned
 *             rows drop out
 *   count   = min(max(k, 0), |S|); out_scores / out_rows as svs_index_search (stride k, order
 *             (score desc, row desc), f32 dot products of the stored row and the stored query)
 * d != index d -> SVS_ERR_SHAPE; nrows < 0 -> SVS_ERR_INVALID; nrows == 0 or k <= 0 -> count 0,
 * nothing launched.  Only the listed rows are read (a subset of m rows costs about m / n of a corpus
 * pass; each row once per group of queries), and a query's results do not depend on nq.  Blocks;
 * re-entrant on one handle.  Rows of more than 16 KiB -> SVS_ERR_UNSUPPORTED. */
int32_t svs_index_search_rows(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                              const int64_t* rows, int64_t nrows,
                              float* out_scores, int64_t* out_rows, int32_t* out_count);

/* Segmented filtered search: MANY row lists in one call, each with its own query -- the drill-down of a document
 * tree (one query, the children of each of the 50-500 best sections) and per-request scopes (one list per query),
 * which are otherwise a host loop of svs_index_search_rows: a validation, an upload, two or more small launches
 * and a stream synchronisation per list.
 *   rows, seg_begin   segment s is the list rows[seg_begin[s] .. seg_begin[s+1]) (seg_begin has nseg + 1 entries,
 *                     seg_begin[0] == 0, never decreasing); GLOBAL rows in any order, duplicates allowed,
 *                     tombstoned rows drop out, as svs_index_search_rows.  The same row may appear in any
 *                     number of segments.
 *   seg_query         segment s is searched with query seg_query[s]; NULL: with query s, and nseg must equal nq.
 * Exact definition.  At out_*[s*k .. s*k + out_counts[s]) the result is what
 *   svs_index_search_rows(idx, queries + seg_query[s]*d, 1, d, k, rows + seg_begin[s], seg_begin[s+1] - seg_begin[s], ...)
 * writes: the same rows, order (score desc, row desc) and score bits; out_counts[s] = min(max(k, 0), live listed
 * rows of s, duplicates collapsed); entries past the count are not touched.  Nothing is grouped, merged or
 * deduplicated ACROSS segments, and a segment's result does not depend on which other segments are in the call, or
 * on their order.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d
 * -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nseg < 0, seg_begin[0] != 0, a decreasing seg_begin, a seg_query entry
 * outside [0, nq), seg_query == NULL with nseg != nq, a row outside [row_offset, row_offset + n) (the message
 * names the first offending segment and row), a null output with work to do.  Rows of more than 16 KiB, or 2^31
 * or more live rows in the segments of up to 4096 rows -> SVS_ERR_UNSUPPORTED.  nseg == 0, k <= 0 or no live
 * listed row anywhere -> SVS_OK, all written counts 0, nothing launched.
 * The segments of 1 .. 4096 live rows are scored by ONE launch and ranked by one more, their rows mapped on the
 * device; a larger segment is served inside the same call by svs_index_search_rows' own kernels.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer: all as svs_index_search_rows.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, coalescing concurrent filtered callers
 * into one segmented call; svs_index_search_rows, its kernels and the top-k stage are unchanged. */
int32_t svs_index_search_segments(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                                  const int64_t* rows, const int64_t* seg_begin /* nseg + 1 */,
                                  const int32_t* seg_query /* nseg, or NULL */, int32_t nseg,
                                  float* out_scores, int64_t* out_rows, int32_t* out_counts /* nseg */);

/* ---- labels: one uint32_t per row, kept next to the vectors in HBM, and the search that names them -- "one level of
 *      the document tree", "one tenant", "one source" -- for which a row list (svs_index_search_rows) is the wrong
 *      tool: at 1M rows the list's SQL, validation and upload cost more than the search.
 * The column.  HBM only (no host mirror), one label per row of the index's row CAPACITY, counted in hbm_bytes.  A row
 * that was never labelled carries label 0, and an index on which svs_index_set_labels was never called behaves as if
 * every label were 0 and owns no column.  The first svs_index_set_labels (with nrows > 0) allocates it, zero-filled;
 * svs_index_reserve, svs_index_append* and svs_index_staging_commit carry it along when the buffers grow, and new
 * rows get label 0; svs_index_mask_rows does not touch it; svs_index_compact moves it with the rows (new row p carries
 * the label of the row it was) -- the compacted column is built in a fresh buffer BEFORE the first row moves, so no
 * memory for it is SVS_ERR_NOMEM with the handle untouched, like the bounce buffer.
 *   set: labels[0 .. nrows) become the labels of GLOBAL rows [row0, row0 + nrows); tombstoned rows may be labelled.
 *        Holds a reference and the geometry lock exclusively, like svs_index_mask_rows: it waits for what it would
 *        disturb, and a search never sees half of one call's range.
 *   get: reads the DEVICE copy of those rows' labels back (zeros when the index has no column); tombstoned rows too.
 * Both: nrows < 0, or a range that is not inside [row_offset, row_offset + n) -> SVS_ERR_INVALID; null labels / out
 * with nrows > 0 -> SVS_ERR_INVALID; nrows == 0 -> SVS_OK, nothing allocated, nothing read.
 *
 * Labelled search.  Exact definition: let S = { live local rows r : label[r] in set(labels) }, ascending.  The call
 * writes what
 *   svs_index_search_rows(idx, queries, nq, d, k, S + row_offset, |S|, ...)
 * writes: the same rows, the same order (score desc, row desc), the same score bits, the same *out_count =
 * min(max(k, 0), |S|); entries past the count are not touched.  *out_matched (may be NULL) = |S|; *out_count (may be
 * NULL) and *out_matched are written by every successful call.  A query's result does not depend on nq.
 *   labels    any order, repeats allowed: sorted and deduplicated on the host.  nlabels == 0 is the empty set: SVS_OK,
 *             count 0, matched 0, nothing launched.
 *   COUNT-ONLY call: with out_matched != NULL and (k <= 0 or nq == 0) only the counting launch runs; out_scores /
 *             out_rows may be NULL.  With out_matched == NULL and (k <= 0 or nq == 0): SVS_OK, nothing launched.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE, as svs_index_search_rows.  SVS_ERR_INVALID: nq < 0, nlabels < 0, null labels with
 * nlabels > 0, null queries with nq > 0, null out_scores / out_rows with work to do (nq > 0, k > 0 and a set that is
 * not empty).  More than SVS_LABELS_MAX_SET DISTINCT labels -> SVS_ERR_UNSUPPORTED (repeats do not count).  Rows of
 * more than 16 KiB with work to do -> SVS_ERR_UNSUPPORTED, the gather kernels' limit.
 * Cost: the filter runs on the device -- a counting pass over the column (4 bytes per row; the set in LDS, a set of
 * one label a plain compare), ONE host wait for |S|, then a one-workgroup scan and a writing pass that emit S in
 * ascending order; then svs_index_search_rows' own score and top-k kernels over that device list (always the list
 * route, whatever the share of rows that match), and the result positions are mapped to rows on the device.  No
 * list is built, checked, sorted or uploaded on the host.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_search_rows.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, per-query label sets in one call,
 * predicates richer than set membership (ranges, bit masks), and routing very broad sets through a full-corpus pass
 * instead of the list route. */
#define SVS_LABELS_MAX_SET 1024
int32_t svs_index_set_labels(svs_index* idx, int64_t row0 /* GLOBAL */, int64_t nrows, const uint32_t* labels);
int32_t svs_index_get_labels(svs_index* idx, int64_t row0 /* GLOBAL */, int64_t nrows, uint32_t* out);
int32_t svs_index_search_labeled(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                                 const uint32_t* labels, int32_t nlabels,
                                 float* out_scores, int64_t* out_rows /* stride k */,
                                 int32_t* out_count, int64_t* out_matched /* or NULL */);

/* ---- columns and predicate search: up to SVS_COLUMNS_MAX uint32_t columns per row and a top-k under a conjunction of
 *      predicates over them -- "this tenant AND this date range", "this level AND a child of these parents", "visible
 *      to any of my groups AND not already seen" -- without a host row list.
 * Columns.  Column 0 IS the label column above: svs_index_set_column(idx, 0, ...) and svs_index_set_labels write the
 * same memory, and every label entry reads column 0.  Columns 1 .. SVS_COLUMNS_MAX - 1 follow the label column's
 * rules word for word, each on its own: HBM only, one u32 per row of the row CAPACITY (rounded up to 4 rows), counted
 * in hbm_bytes; null until first set -- a row never set reads 0, and the rows from n on are 0; allocated zero-filled by
 * the first svs_index_set_column with nrows > 0 (no memory -> SVS_ERR_NOMEM, handle untouched); svs_index_reserve,
 * svs_index_append* and svs_index_staging_commit carry it along when the buffers grow and new rows get 0;
 * svs_index_mask_rows does not touch it; svs_index_compact moves it with the rows, every compacted column built in a
 * fresh buffer BEFORE the first row moves (no memory for any of them -> SVS_ERR_NOMEM, handle untouched); tombstoned
 * rows may be written and read.  set holds a reference and the geometry lock exclusively, get holds it shared.
 * column outside [0, SVS_COLUMNS_MAX) -> SVS_ERR_INVALID; range and null-pointer rules: svs_index_set_labels /
 * svs_index_get_labels.  A column never set costs nothing and stays unallocated through growth and compaction.
 *
 * Predicate search.  A term is true on a row when its op holds on v = column[term.column][row], inverted when
 * negate == 1:
 *   SVS_WHERE_IN        v is a member of set[0 .. nset) (host; any order, repeats allowed; an empty set is never true)
 *   SVS_WHERE_RANGE     a <= v && v <= b                (a > b: never true)
 *   SVS_WHERE_ANY_BITS  (v & a) != 0
 *   SVS_WHERE_ALL_BITS  (v & a) == a
 * Exact definition: let S = { live local rows r : every term is true on r }, ascending; nterms == 0: every live row.
 * The call writes what
 *   svs_index_search_rows(idx, queries, nq, d, k, S + row_offset, |S|, ...)
 * writes: the same rows, the same order (score desc, row desc), the same score bits, the same *out_count =
 * min(max(k, 0), |S|); entries past the count are not touched.  *out_matched (may be NULL) = |S|; *out_count (may be
 * NULL) and *out_matched are written by every successful call.  A query's result does not depend on nq, on the order
 * of the terms, or on the order and repeats inside a set.  One term {column 0, IN, set} is svs_index_search_labeled
 * with that set, bit for bit, matched included.
 *   COUNT-ONLY call: with out_matched != NULL and (k <= 0 or nq == 0) only the counting launch runs; out_scores /
 *             out_rows may be NULL.  With out_matched == NULL and (k <= 0 or nq == 0): SVS_OK, nothing launched.
 *             The host takes no other short-cut: a predicate nothing satisfies is found by the counting launch, and the
 *             call ends after it.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nq < 0, nterms < 0, null terms with nterms > 0, a column outside
 * [0, SVS_COLUMNS_MAX), an unknown op, negate not 0 or 1, IN with nset < 0 or a null set with nset > 0, null queries
 * with nq > 0, null out_scores / out_rows with work to do (nq > 0 and k > 0).  SVS_ERR_UNSUPPORTED: nterms >
 * SVS_WHERE_MAX_TERMS; more than SVS_LABELS_MAX_SET distinct set members summed over the call's IN terms (each term's
 * repeats do not count; one 4 KiB LDS image holds all sets); rows of more than 16 KiB with work to do.
 * Cost: a counting pass that reads 4 bytes per row of every DISTINCT column the terms name plus one bit per row (a
 * column the index does not own is not read), ONE host wait for |S|, a one-workgroup scan and a writing pass that
 * reads the same again and emits S in ascending order (svs_amd/csrc/where.h); then svs_index_search_rows' own score
 * and top-k kernels over that device list and the mapping of positions to rows on the device -- the path of
 * svs_index_search_labeled from there on.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, OR across terms, per-query predicates in
 * one call, 64-bit or float columns, more than four columns or terms, routing broad predicates through a full-corpus
 * pass, columns on the attach path. */
#define SVS_COLUMNS_MAX 4          /* column 0 IS the label column of svs_index_set_labels */
#define SVS_WHERE_MAX_TERMS 4
typedef enum svs_where_op { SVS_WHERE_IN = 0, SVS_WHERE_RANGE = 1, SVS_WHERE_ANY_BITS = 2, SVS_WHERE_ALL_BITS = 3 } svs_where_op;
typedef struct svs_where_term_t {
  int32_t column;        /* 0 .. SVS_COLUMNS_MAX-1; a column never set reads 0 everywhere */
  int32_t op;            /* svs_where_op */
  int32_t negate;        /* 0 / 1: the term is the op's truth value, inverted when 1 */
  uint32_t a, b;         /* RANGE: a <= v && v <= b (a > b: never true); ANY_BITS: (v & a) != 0; ALL_BITS: (v & a) == a; IN: unused */
  const uint32_t* set;   /* IN: host, any order, repeats allowed; others: ignored */
  int32_t nset;          /* IN: >= 0; an empty set is never true */
} svs_where_term_t;
int32_t svs_index_set_column(svs_index* idx, int32_t column, int64_t row0 /* GLOBAL */, int64_t nrows, const uint32_t* values);
int32_t svs_index_get_column(svs_index* idx, int32_t column, int64_t row0 /* GLOBAL */, int64_t nrows, uint32_t* out);
int32_t svs_index_search_where(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                               const svs_where_term_t* terms, int32_t nterms,
                               float* out_scores, int64_t* out_rows /* stride k */,
                               int32_t* out_count, int64_t* out_matched /* or NULL */);

/* Threshold search: every live row that scores at or above a cut-off, best first, and how many there are -- "all
 * documents with cosine >= 0.8", "how many would qualify", "drop the weak tail by score, not by rank" -- without
 * guessing a k and without pulling the score vector to the host.
 * Exact definition.  For query q of the call let s be the vector svs_index_scores_n(idx, query q) returns at that
 * moment (the unscreened single-query score kernel of the index's dtype), L the live (not tombstoned) local rows, and
 *   A = { r in L : score_key(s[r]) >= score_key(min_scores[q]) }
 * with the orderable key of the top-k order (svs_amd/csrc/keys.h).  The comparison is made in KEY space, the space the
 * order is defined in: -0.0 and +0.0 are one value; a NaN SCORE maps to the largest key, so it qualifies for every
 * cut-off and sorts first, exactly as in svs_index_search; a cut-off of -inf admits every live row.  Tombstoned rows are
 * excluded by the dead-row bitmap, never by their score.
 *   out_totals[q]   = |A|, always exact, also beyond `limit` and beyond every internal capacity; may be NULL
 *   out_counts[q]   = min(max(limit, 0), |A|)
 *   out_*[q*limit .. q*limit + out_counts[q])   the first out_counts[q] elements of A in descending
 *                     make_key(s[r], r), that is (score desc, row desc): scores are the bits of s, rows are
 *                     row_offset + r (a NaN comes back as the quiet NaN 0x7fc00000, as from every search); entries
 *                     past the count are not touched
 * A query's result does not depend on nq, on the other queries of the call or on their order.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nq < 0, null queries or min_scores with nq > 0, a NaN in
 * min_scores (the message names the query), null out_counts, null out_scores / out_rows with limit > 0 and nq > 0.
 * limit <= 0 is a COUNT-ONLY call: the totals are computed, every count is 0, out_scores / out_rows may be NULL --
 * the one place where a non-positive limit still launches work.  nq == 0 -> SVS_OK, nothing launched.
 * Each query costs one single-query corpus pass plus two small launches (a filter over the score vector, one
 * workgroup that orders the survivors); up to 32,768 qualifying rows with min(limit, total) <= 4096 are finished on
 * the device, beyond that the query is re-run through the exact top-k stage with k = min(limit, total) after the
 * call's one wait: the same answer by definition.  (In that re-run a LIVE row whose score is -inf itself ties with the
 * masked rows; finite rows and queries never produce one.)
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_scores_n and
 * svs_index_search_rows.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, the batched GEMM score routes (every
 * query is one single-query pass), and the screened route: an f32 index reads its f32 rows here, not the half shadow
 * (screening a cut-off with the shadow's error bound is the natural follow-up). */
int32_t svs_index_search_above(svs_index* idx, const float* queries, int32_t nq, int32_t d,
                               const float* min_scores /* nq */, int32_t limit,
                               float* out_scores, int64_t* out_rows /* stride limit */,
                               int32_t* out_counts /* nq */, int64_t* out_totals /* nq, or NULL */);

/* Combined search: the top k rows ranked by how they score against SEVERAL vectors at once -- the best score against
 * any of a question's rewordings (MAX), "relevant to all of these" (MIN), "like these, less like those" (a weighted SUM
 * with negative weights) -- in one pass over the corpus and one selection, with nothing but the answer leaving the device.
 * Exact definition.  A combined query is m vectors v_0 .. v_{m-1} (1 <= m <= SVS_COMBINE_MAX_VECTORS), weights w_j
 * (weights == NULL: every w_j is 1.0f) and an op.  Let s_j be the vector svs_index_scores_n(idx, v_j) returns at that
 * moment (the unscreened single-query score kernel of the index's dtype: each vector is quantised the way the index
 * quantises a query; an f32 index reads its f32 rows, never the half shadow), and t_j[i] = w_j * s_j[i], ONE f32
 * multiplication rounded to nearest (with w_j == 1.0f that is s_j[i]).  The combined score c[i] of local row i is
 *   SVS_COMBINE_MAX   key_score(max_j score_key(t_j[i]))    the order's own key (svs_amd/csrc/keys.h): -0.0 folds onto
 *   SVS_COMBINE_MIN   key_score(min_j score_key(t_j[i]))    +0.0 and any NaN is the largest value
 *   SVS_COMBINE_SUM   ((t_0[i] + t_1[i]) + t_2[i]) + ...    f32 additions in vector order, each rounded to nearest; no
 *                                                           fused multiply-add joins a multiplication and an addition
 * and the result is what the top-k stage returns over c with the tombstoned rows masked: count = min(max(k, 0), live
 * rows), out_*[q*k .. q*k + count) in (score desc, row desc) order, rows as row_offset + local row, a NaN as the quiet
 * NaN 0x7fc00000; entries past the count are not touched.  *out_count (may be NULL) is the same for every query.  With
 * m == 1, weights == NULL and SVS_COMBINE_MAX the result equals svs_index_search's on an unscreened index: rows and
 * score bits.  A query's result does not depend on nq or on the other queries of the call.
 * vectors: host, (nq, m, d) C-contiguous; weights: host, (nq, m), or NULL.  The nq combined queries run back to back
 * on one stream with no host wait between them.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  All of them are
 * SVS_ERR_INVALID and name the argument: nq < 0, m outside 1 .. SVS_COMBINE_MAX_VECTORS, d != index d, an unknown op,
 * k < 0, null vectors with nq > 0, a NaN or infinite weight (the message names the query and the vector), null
 * out_scores / out_rows with work to do (nq > 0 and count > 0).  nq == 0 or k == 0 -> SVS_OK, nothing launched.
 * Cost.  Row lengths with a one-shot single-query kernel (f32: multiples of 256 floats up to 4096; f16: multiples of
 * 512 halves up to 4096; fp8: 512, 1024, 1536, 2048, 3072, 4096 bytes) take ONE fused pass: every wave loads its rows
 * once and streams the m vectors through them.  Every other row length takes m single-query passes and one elementwise
 * kernel over the m score vectors.  Both give the bits of the definition.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_search_above.
 * Out of scope: svs_multi / row-sharded corpora and a device-pointer variant. */
#define SVS_COMBINE_MAX_VECTORS 8
enum { SVS_COMBINE_MAX = 0, SVS_COMBINE_MIN = 1, SVS_COMBINE_SUM = 2 };
int32_t svs_index_search_combined(svs_index* idx, const float* vectors /* host, [nq][m][d] */, int32_t nq, int32_t m, int32_t d,
                                  const float* weights /* [nq][m] or NULL */, int32_t op, int32_t k,
                                  float* out_scores, int64_t* out_rows /* [nq][k] */, int32_t* out_count);

/* Per-label breakdown: for every label of a set, how many live rows of that label score at or above a cut-off and
 * which of them is the best, the labels ordered by their best row -- facet counts plus one best hit per facet ("120
 * hits in manuals, 30 in FAQ, 2 in release notes; here is the best one of each, best source first") in one corpus
 * pass per query, whatever the number of labels.
 * Exact definition.  For query q of the call let s be the vector svs_index_scores_n(idx, query q) returns at that
 * moment (the unscreened single-query score kernel of the index's dtype, the one svs_index_search_above uses), L the
 * live (not tombstoned) local rows, T = score_key(min_scores[q]) (svs_amd/csrc/keys.h; min_scores == NULL: -inf for
 * every query), and for each DISTINCT label l of `labels`
 *   A_l     = { r in L : label[r] == l and score_key(s[r]) >= T }      (an index without a column: label[r] == 0)
 *   G       = { l : A_l is not empty }
 *   best(l) = max over r in A_l of make_key(s[r], r)
 * The comparison is made in KEY space, as in svs_index_search_above: -0.0 and +0.0 are one cut-off; a NaN SCORE
 * qualifies for every cut-off and sorts first; -inf admits every live row.  Tombstoned rows are excluded by the
 * dead-row bitmap, never by their score.
 *   out_groups[q]   = |G|; may be NULL
 *   out_counts[q]   = min(max(k, 0), |G|)
 *   out_*[q*k + t], t < out_counts[q]   the labels of G in descending best(l) -- keys are unique because rows are, so
 *                     the order is total: the top-k order (score desc, row desc) applied to each label's best row.
 *                     out_labels = l, out_scores = the score bits of the best row (a NaN comes back as the quiet NaN
 *                     0x7fc00000), out_rows = row_offset + the best row, out_totals = |A_l|, always exact.  Entries
 *                     past the count are not touched.
 * A query's result does not depend on nq, on the other queries of the call, or on the order and repeats of `labels`
 * (sorted and deduplicated on the host, as svs_index_search_labeled does).  Counts are integers and the best row is the
 * maximum of unique integer keys: the answer is bit-reproducible however the device schedules the work.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nq < 0, nlabels < 0, null labels with nlabels > 0, null queries
 * with nq > 0, a NaN in min_scores (the message names the query), null out_counts, null out_labels / out_scores /
 * out_rows / out_totals with k > 0, nq > 0 and nlabels > 0.  More than SVS_LABELS_MAX_SET DISTINCT labels ->
 * SVS_ERR_UNSUPPORTED.  k <= 0 is a COUNT-ONLY call: out_groups is computed, every count is 0, the four result pointers
 * may be NULL.  nq == 0 or nlabels == 0 -> SVS_OK, counts and groups 0, nothing launched.
 * Each query costs one single-query corpus pass plus two small launches: a reduction over the score vector, the label
 * column and the bitmap (8 bytes per row) into one count and one best key per label, and one workgroup that ranks
 * the at most SVS_LABELS_MAX_SET groups.  The host waits once per call.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_search_above.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, more than one row per label, the batched
 * GEMM and the screened score routes.  (Groups that are not a caller-given set -- one group per parent document --
 * are svs_index_search_collapsed below.) */
int32_t svs_index_search_by_label(svs_index* idx, const float* queries, int32_t nq, int32_t d,
                                  const uint32_t* labels, int32_t nlabels,
                                  const float* min_scores /* nq, or NULL: -inf for every query */, int32_t k,
                                  uint32_t* out_labels, float* out_scores, int64_t* out_rows,
                                  int64_t* out_totals /* all four: stride k */,
                                  int32_t* out_counts /* nq */, int32_t* out_groups /* nq, or NULL */);

/* Collapsed search: the top k rows with at most ONE row per value of a column -- "the 10 best parent documents, each
 * represented by its best chunk" (other vector stores: collapse, group_by) -- in one corpus pass per query, whatever
 * the number of distinct values: a corpus has as many parents as it has documents, and none of them is named in the call.
 * Exact definition.  For query q of the call let s be the vector svs_index_scores_n(idx, query q) returns at that
 * moment (the unscreened single-query score kernel of the index's dtype, the one svs_index_search_above uses), L the
 * live (not tombstoned) local rows and v[r] = column[column][r] (a column never set reads 0 everywhere).  Row r's group
 * is v[r]; under SVS_COLLAPSE_ZERO_SINGLE a row with v[r] == 0 is a group of its own ("no parent" never collapses),
 * under SVS_COLLAPSE_ZERO_IS_GROUP 0 is a value like any other.
 *   best(G) = max over r in G and L of make_key(s[r], r)     (svs_amd/csrc/keys.h)
 *   W       = { r : r is the best of its group }             (a group with no live row has none)
 * The maximum is taken in KEY space, the space the order is defined in: -0.0 folds onto +0.0, a NaN score is the
 * largest, a score tie goes to the larger row, as everywhere.  Tombstoned rows are excluded by the dead-row bitmap,
 * never by their score.
 *   out_groups[q]   = |W|, always exact; may be NULL
 *   out_counts[q]   = min(max(k, 0), |W|)
 *   out_*[q*k + t], t < out_counts[q]   the rows of W in descending key, that is (score desc, row desc): out_scores =
 *                     the score bits of s (a NaN comes back as the quiet NaN 0x7fc00000, as from every search),
 *                     out_rows = row_offset + r, out_values = v[r].  Entries past the count are not touched.
 * A query's result does not depend on nq, on the other queries of the call, or on how the device schedules the work:
 * it is maxima of unique integer keys and an integer count.  Two identities: a column never set gives, under
 * ZERO_SINGLE, the plain top-k over s with the tombstoned rows masked (rows and score bits), and under ZERO_IS_GROUP
 * one hit, the best live row.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nq < 0, a column outside [0, SVS_COLUMNS_MAX), an unknown
 * zero_mode, null queries with nq > 0, null out_counts, null out_scores / out_rows / out_values with k > 0 and nq > 0.
 * k <= 0 is a COUNT-ONLY call: the groups are counted, every count is 0, the three result pointers may be NULL.
 * nq == 0 -> SVS_OK, nothing launched.
 * Each query costs one single-query corpus pass, two passes over the score vector, the column and the bitmap (8 bytes
 * per row each: one finds every group's best key in an open-addressing table in HBM with 64-bit integer compare-and-
 * swap and max -- no float atomics, nothing waits or spins --, one strikes every row that is not its group's best to
 * -inf and counts the rest), a fill that empties the table, the top-k stage with k' = min(k, live rows) over the
 * rewritten vector, and one tiny launch for the values; after the call's one wait the host trims each query to
 * min(k, |W|).  Every row of W sorts above every struck row.  (A LIVE best row whose score is -inf itself ties with
 * the struck rows; finite rows and queries never produce one.)  The table belongs to the search context: 16 bytes per
 * slot, a power of two >= 2 x rows slots -- 32 to 64 MB per million rows and per context that ran a collapsed search.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_search_above.
 * Out of scope: more than one row per group or a per-group row count, grouping by two columns, svs_multi /
 * row-sharded corpora, a device-pointer variant, the batched GEMM and the screened score routes, routing through shared passes. */
enum { SVS_COLLAPSE_ZERO_IS_GROUP = 0, SVS_COLLAPSE_ZERO_SINGLE = 1 };
int32_t svs_index_search_collapsed(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                                   int32_t column, int32_t zero_mode,
                                   float* out_scores, int64_t* out_rows, uint32_t* out_values /* all three: stride k */,
                                   int32_t* out_counts /* nq */, int64_t* out_groups /* nq, or NULL */);

/* Collapsed search inside a scope: svs_index_search_collapsed's groups over the rows of a predicate or of a row list
 * -- "the 10 best documents of tenant 7, one hit per document", "the 10 best chapters, judged by their best level-2
 * section" -- with nothing but the answer leaving the device.  (Over-fetching from svs_index_search_where and
 * de-duplicating is wrong whenever one parent holds the best rows.)
 * Exact definition.  The scope S, ascending:
 *   _where   S = { live local rows r : every term is true on r }: svs_index_search_where's S, with its term semantics
 *            and limits; nterms == 0: every live row
 *   _rows    S = the live rows of `rows` (GLOBAL, any order, repeats allowed), ascending, each once:
 *            svs_index_search_rows' S
 * For query q of the call and r in S let t[r] = the score bits svs_index_search_rows reports for row r when called
 * with that query over S + row_offset and k = |S|: the GATHER kernel's score, not svs_index_scores_n's.  v[r] =
 * column[column][r] (a column never set reads 0 everywhere); groups, the two zero modes and make_key are
 * svs_index_search_collapsed's, restricted to S:
 *   best(G) = max over r in G and S of make_key(t[r], r)     (svs_amd/csrc/keys.h)
 *   W       = { r : r is the best of its group }             (a group with no row in S has none)
 *   *out_matched    = |S|; may be NULL
 *   out_groups[q]   = |W|, always exact; may be NULL
 *   out_counts[q]   = min(max(k, 0), |W|)
 *   out_*[q*k + t], t < out_counts[q]   the rows of W in descending key, that is (score desc, row desc): out_scores =
 *                     the score bits of t (a NaN comes back as the quiet NaN 0x7fc00000, as from every search),
 *                     out_rows = row_offset + r, out_values = v[r].  Entries past the count are not touched.
 * A query's result does not depend on nq, on the other queries of the call, or on how the device schedules the work.
 * Three identities.  (a) A column never set under ZERO_SINGLE gives svs_index_search_where's / svs_index_search_rows'
 * result -- rows and score bits -- with groups = |S|.  (b) A column never set under ZERO_IS_GROUP gives one hit, the
 * first row of (a).  (c) The two entries agree bit for bit when `rows` lists exactly the predicate's S.
 * NOT claimed: any identity with the unscoped svs_index_search_collapsed, not even with nterms == 0 -- that entry
 * collapses the full-pass kernel's scores, these collapse the gather kernel's, and the two need not round alike.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: svs_index_search_collapsed's argument errors (nq < 0, a column
 * outside [0, SVS_COLUMNS_MAX), an unknown zero_mode, null queries with nq > 0, null out_counts, null out_scores /
 * out_rows / out_values with k > 0 and nq > 0); _where: svs_index_search_where's term errors (nterms < 0, null terms
 * with nterms > 0, a term's column outside [0, SVS_COLUMNS_MAX), an unknown op, negate not 0 or 1, IN with nset < 0 or
 * a null set with nset > 0); _rows: svs_index_search_rows' list errors (nrows < 0, null rows with nrows > 0, a row
 * outside the index).  SVS_ERR_UNSUPPORTED: nterms > SVS_WHERE_MAX_TERMS; more than SVS_LABELS_MAX_SET distinct set
 * members over the call's IN terms; rows of more than 16 KiB with work to do (nq > 0).
 * nq == 0 -> SVS_OK, nothing launched, nothing written.  |S| == 0 -> SVS_OK, counts and groups 0, matched 0; nothing
 * runs after the counting launch (_rows: nothing runs).  k <= 0 is a COUNT-ONLY call, as in
 * svs_index_search_collapsed: groups and matched are computed, every count is 0, the three result pointers may be NULL.
 * Cost.  _where: svs_index_search_where's counting pass and ONE host wait for |S|, then a one-workgroup scan and ONE
 * writing pass that evaluates the predicate once and emits both S and the group column compacted beside it (one more
 * 16-byte load per lane and step; none when a term names the column anyway or the index does not own it).  _rows: the
 * list is built on the host and uploaded as svs_index_search_rows does, and a tiny launch reads its column values.
 * Then the gather kernel scores the list for chunks of queries whose score vectors stay <= 2 GiB, and every query's
 * |S| scores go through svs_index_search_collapsed's own kernels with list positions for rows (positions ascend with
 * rows, so a tie still goes to the larger row): reduce, mark, the table's fill -- a table sized by |S|, not by the
 * index --, the top-k stage, the values; positions become rows on the device (svs_amd/csrc/collapse_scope.h).
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; two host waits per call (_rows: one); never goes through the coalescer, the run-ahead pipelines or shared
 * passes: all as svs_index_search_where.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, a scoped
 * svs_index_search_collapsed_combined, svs_index_search_above and svs_index_search_by_label under a scope, OR across
 * terms, routing a broad predicate through a full-corpus pass. */
int32_t svs_index_search_collapsed_where(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                                         const svs_where_term_t* terms, int32_t nterms,
                                         int32_t column, int32_t zero_mode,
                                         float* out_scores, int64_t* out_rows, uint32_t* out_values /* stride k */,
                                         int32_t* out_counts /* nq */, int64_t* out_groups /* nq, or NULL */,
                                         int64_t* out_matched /* or NULL */);
int32_t svs_index_search_collapsed_rows(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k,
                                        const int64_t* rows, int64_t nrows,
                                        int32_t column, int32_t zero_mode,
                                        float* out_scores, int64_t* out_rows, uint32_t* out_values,
                                        int32_t* out_counts, int64_t* out_groups, int64_t* out_matched);

/* Group-combined search: the top k GROUPS (parent documents) ranked against several vectors at once, where a group's
 * score against each vector is its best row's -- "the documents that cover both facets, wherever in the document":
 * chunk 3 may answer the first facet and chunk 9 the second.  svs_index_search_combined combines per ROW (one chunk
 * must cover everything); svs_index_search_collapsed takes one vector.  This is their product, per group.
 * Exact definition.  For combined query q (m vectors, weights, op: svs_index_search_combined's) let s_j be the vector
 * svs_index_scores_n(idx, v_j) returns at that moment (the unscreened single-query kernel of the index's dtype), L
 * the live local rows and v[r] = column[column][r].  Groups and the two zero modes are svs_index_search_collapsed's:
 * row r's group is v[r]; under SVS_COLLAPSE_ZERO_SINGLE a row with v[r] == 0 is a group of its own.
 *   M_j(G) = max over r in G and L of score_key(s_j[r])       a 32-bit key (svs_amd/csrc/keys.h), of the UNWEIGHTED
 *                                                              score: the chunk of G that matches vector j best
 *   c(G)   = combine_finish(fold over j = 0 .. m-1 of combine_step(acc, key_score(M_j(G)), w_j, op), op), from
 *            combine_init(op): svs_amd/csrc/combine.h's one implementation of MAX, MIN and SUM over the m per-vector
 *            maxima; t_j = w_j * key_score(M_j) is ONE f32 multiplication, the additions run in vector order and are
 *            never contracted into a fused multiply-add; weights == NULL: every weight is 1.0f
 *   rep(G) = the row of G and L with the largest make_key(c_row[r], r), c_row = svs_index_search_combined's per-row
 *            combined score for the same vectors, weights and op: the row the row-level search would rank first
 *   W      = the groups that have a live row
 *   out_groups[q]   = |W|, always exact; may be NULL
 *   out_counts[q]   = min(max(k, 0), |W|)
 *   out_*[q*k + t], t < out_counts[q]   the groups in descending make_key(c(G), rep(G)): out_scores = c(G) (a NaN comes
 *                     back as the quiet NaN 0x7fc00000, -0.0 as +0.0, as from every search), out_rows = row_offset +
 *                     rep(G), out_values = v[rep(G)].  Entries past the count are not touched.
 * Every reduction is a maximum of integer keys or a fixed-order f32 chain over m numbers: the answer is bit-reproducible
 * and does not depend on nq, on the other queries of the call or on how the device schedules the work.
 * Three identities.  (1) m == 1, weights == NULL, SVS_COMBINE_MAX: svs_index_search_collapsed's result -- rows, values,
 * groups and score bits.  (2) Every group a single row (a column never set under ZERO_SINGLE): svs_index_search_combined's
 * result for every op and weight (a score of -0.0 arrives canonicalised as +0.0 at every stage).  (3) SVS_COMBINE_MAX with
 * all weights >= 0: collapsing the row-level combined vector -- the multiplication is monotone, so the maximum over rows
 * and the maximum over vectors commute.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  All are
 * SVS_ERR_INVALID and name this function: nq < 0, m outside 1 .. SVS_COMBINE_MAX_VECTORS, d != index d, an unknown op,
 * null vectors with nq > 0, a NaN or infinite weight, a column outside [0, SVS_COLUMNS_MAX), an unknown zero_mode, null
 * out_counts, null out_scores / out_rows / out_values with k > 0 and nq > 0.  k <= 0 is a COUNT-ONLY call: the groups
 * are counted, every count is 0, the three result pointers may be NULL.  nq == 0 -> SVS_OK, nothing launched; an empty
 * index -> SVS_OK, counts and groups 0, nothing launched.
 * Cost per combined query.  The score pass: row lengths with a one-shot single-query kernel (see
 * svs_index_search_combined) take ONE fused multi-score pass -- every wave loads its rows once, streams the m vectors
 * through them and stores m scores per row --, every other row length m single-query passes.  Then two passes over the m
 * score vectors, the column and the bitmap (4 m + 4 bytes per row each): one finds every group's slot in
 * svs_index_search_collapsed's open-addressing table and raises its representative key (64-bit integer max) and its m
 * per-vector keys (32-bit integer max; no float atomics, nothing waits or spins), one writes c(G) at every representative
 * row and -inf everywhere else and counts; two fills; the top-k stage with k' = min(k, live rows); one tiny launch for
 * the values.  The host waits once per call.  (A group whose c(G) is -inf itself ties with the struck rows, as in
 * svs_index_search_collapsed.)  Memory per search context: the collapsed search's table (16 bytes per slot) plus 4 bytes
 * per slot and vector, a power of two >= 2 x rows slots -- per million rows 2^21 slots, 32 MB + 8 MB per vector: 40 MB
 * at m = 1, 96 MB at m = 8 (up to twice that just above a power of two); m score vectors of 4 bytes per row.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer, the run-ahead pipelines or shared passes: all as svs_index_search_above.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, more than SVS_COMBINE_MAX_VECTORS vectors,
 * mean or count aggregates over a group, predicates and row lists, the screened and the batched GEMM score routes. */
int32_t svs_index_search_collapsed_combined(svs_index* idx, const float* vectors /* host, [nq][m][d] */, int32_t nq, int32_t m, int32_t d,
                                            const float* weights /* [nq][m] or NULL */, int32_t op /* SVS_COMBINE_* */, int32_t k,
                                            int32_t column, int32_t zero_mode /* SVS_COLLAPSE_ZERO_* */,
                                            float* out_scores, int64_t* out_rows, uint32_t* out_values /* all three: stride k */,
                                            int32_t* out_counts /* nq */, int64_t* out_groups /* nq, or NULL */);

/* Nearest-vector assignment: for every stored row of a range, which of c given vectors it scores best against -- the
 * transposed question of a search ("which topic is each document about", the assignment step of a clustering, coarse
 * centroids for probing), answered where the corpus lies; optionally the answer is written into the label column, so
 * that svs_index_search_labeled and svs_index_search_by_label then work per topic or cluster.
 * Exact definition.
 *   Vectors as stored.  V[j] is vector j as a stored row of an index of this handle's dtype -- what
 *     svs_index_debug_query returns for it: f32 unchanged, f16 rounded to half, fp8 e4m3 with its own scale.  The
 *     vectors go through the rows' ingest and quantisation kernels.  Nothing requires unit norm.
 *   Score of a pair.  For local row r and position j, A[r][j] = the dot product of the STORED values of row r and of
 *     V[j], f32 products accumulated in f32 over the columns in ascending order as ONE fmaf chain per element; fp8 sums
 *     the e4m3 values and multiplies by (scale_r * scale_j) once, after the sum (svs_index_search_diverse's rule for G).
 *     A[r][j] depends only on the row's stored values, the vector's stored values and d -- not on c, j, the range,
 *     tiles or scheduling.
 *   Best position.  best[r] = the j that maximises score_key(A[r][j]) (svs_amd/csrc/keys.h); an exact tie in key space
 *     goes to the LOWER j; -0.0 and +0.0 are one value; a NaN score has the largest key, as in every search.
 *   Per-row outputs, for every row of [row0, row0 + nrows) (GLOBAL rows), live or tombstoned, at i = row - row0:
 *     out_best[i] = best, out_scores[i] = key_score(score_key(A[r][best])): the score's bits, -0.0 reported as +0.0, a
 *     NaN as the quiet NaN 0x7fc00000.  Either may be NULL.
 *   Counts.  out_counts[j] = the number of LIVE rows of the range with best == j; the dead-row bitmap decides, never the
 *     score; the counts sum to the live rows of the range.  May be NULL.
 *   Label column.  With vector_labels != NULL, label[r] = vector_labels[best[r]] for every row of the range, tombstoned
 *     rows included (as svs_index_set_labels may label them); labels outside the range are untouched.  The first such
 *     call allocates the zero-filled column exactly as svs_index_set_labels does (counted in hbm_bytes; no memory ->
 *     SVS_ERR_NOMEM, handle untouched).  With vector_labels == NULL the column is neither read, written nor allocated.
 * Scores are single chains, the arg-max is over unique integer keys and the counts are integers: the answer is
 * bit-reproducible however the device schedules the work.
 * Errors: everything is validated before anything is launched; a failing call writes no output and allocates no
 * column.  d != index d or an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: c <= 0, nrows < 0, null vectors, a range
 * not inside [row_offset, row_offset + n).  c > SVS_ASSIGN_MAX_VECTORS -> SVS_ERR_UNSUPPORTED.  nrows == 0 -> SVS_OK,
 * out_counts zeroed if given, nothing launched, no column.  All three outputs NULL and vector_labels == NULL -> SVS_OK,
 * nothing launched.
 * Cost: the c vectors are ingested into a device image of at most 1024 rows (it stays in cache), then ONE kernel
 * streams the range's rows past it (exact f32 MFMA, svs_amd/csrc/assign.h): the rows are read once per 256 vectors (once
 * in all for c <= 256), 2 nrows ld max(c, 64) FLOP; 8 bytes per row come back.
 * Blocking; re-entrant on one handle; holds a reference; waits for pending staging copies; never goes through the
 * coalescer, the run-ahead pipelines or shared passes.  With vector_labels == NULL it holds the geometry lock shared,
 * like a search.  With vector_labels != NULL it holds the geometry lock EXCLUSIVELY for the whole call, as
 * svs_index_set_labels does: searches, appends and other writers on the handle wait that long.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, more than one position per row (soft
 * assignment), more than SVS_ASSIGN_MAX_VECTORS vectors, a second label column.  (Per-label sums, the update step of
 * k-means, are svs_index_label_sums below.) */
#define SVS_ASSIGN_MAX_VECTORS 1024   /* = SVS_LABELS_MAX_SET: every label an assignment writes can be named in one labelled call */
int32_t svs_index_assign(svs_index* idx, const float* vectors /* host, f32, C-contiguous (c, d) */, int32_t c, int32_t d,
                         int64_t row0 /* GLOBAL */, int64_t nrows,
                         const uint32_t* vector_labels /* c, or NULL: the label column is not touched */,
                         int32_t* out_best /* nrows, or NULL */, float* out_scores /* nrows, or NULL */,
                         int64_t* out_counts /* c, or NULL */);

/* Per-label row sums: for every label of a set, the f64 sum of the stored values of the live rows of a range that
 * carry it, and how many there are -- topic centroids, a refined centroid after a classification, and the update step
 * of k-means beside svs_index_assign, computed where the corpus lies: nlabels x d numbers come back instead of every
 * row.
 * Exact definition.
 *   Labels.  The label of local row r is lab[r]: with row_labels != NULL, row_labels[r - r0] (r0 = the range's first
 *     local row; e.g. the out_best of an assignment); otherwise the label column's value, and 0 everywhere for an index
 *     without a column, as everywhere else.
 *   Rows of a label.  For each position j of `labels`, R_j = the LIVE rows of the range with lab[r] == labels[j], in
 *     ascending order r_0 < ... < r_(m-1).  The dead-row bitmap decides which rows are live, never a value.
 *   Values.  x(r)[col] = the stored value as svs_index_debug_dequant returns it, widened to f64 (exact): f32 as is,
 *     f16 the half widened, fp8 the e4m3 value times the row's scale as ONE f32 product.
 *   The sum is a fixed tree of plain IEEE f64 additions; nothing is fused, nothing is reassociated:
 *     chunk t of R_j is the rows r_(256 t) .. r_(min(256 t + 255, m - 1))     (SVS_LABEL_SUMS_CHUNK = 256)
 *     P_t[col] = (((+0.0 + x(r_a)[col]) + x(r_(a+1))[col]) + ...)             one chain over the chunk's rows
 *     S_j[col] = (((+0.0 + P_0[col]) + P_1[col]) + ...)                       one chain over the label's chunks
 *   out_sums[j * d + col] = S_j[col] for col < d (padding columns never appear); out_counts[j] = m.  An empty R_j gives
 *     +0.0 everywhere and count 0; no element is ever -0.0.  Repeated labels are allowed and every position gets its
 *     label's answer: the device works on the sorted distinct set, as svs_index_search_by_label does, and the host
 *     copies each label's answer to the caller's positions.
 * The answer depends only on the stored values, the labels, the bitmap and the range -- not on nlabels, on the other
 * labels of the set, on grids or on scheduling: it is bit-reproducible.  Whenever every partial sum is representable in
 * f64 the result is the exact sum; that holds for all f16 data of realistic size and for unit-norm f32 data.
 * Errors: everything is validated before anything is launched, and a failing call writes nothing.  An empty index ->
 * SVS_ERR_SHAPE.  SVS_ERR_INVALID: nlabels < 0, nrows < 0, null labels with nlabels > 0, a range not inside
 * [row_offset, row_offset + n).  More than SVS_LABELS_MAX_SET DISTINCT labels -> SVS_ERR_UNSUPPORTED.  Rows of more
 * than 16 KiB (the gather kernels' limit) when sums are asked for over a non-empty range and set -> SVS_ERR_UNSUPPORTED.
 * nlabels == 0, or both outputs NULL -> SVS_OK, nothing launched.  nrows == 0 -> SVS_OK, the given outputs zeroed,
 * nothing launched.  out_sums == NULL with out_counts given is a COUNT-ONLY call: only the histogram runs, and no row
 * is read.
 * Cost: two passes over 4 bytes of label and one bit per row of the range (a histogram per strip of rows, then a
 * stable scatter into a label-major row list), then every matching row is read ONCE (svs_amd/csrc/label_sums.h); the
 * chunks' partial sums, (ceil(nrows / 256) + nlabels) x d f64 at most, are written and folded on the device.  The host
 * waits once per call; row_labels (4 bytes per row) goes up, nlabels x d f64 and the counts come back.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared, like a search and like
 * svs_index_assign without labels; waits for pending staging copies; never goes through the coalescer, the run-ahead
 * pipelines or shared passes; never allocates a label column.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, weighted sums, sums of squares. */
#define SVS_LABEL_SUMS_CHUNK 256   /* part of the definition above */
int32_t svs_index_label_sums(svs_index* idx, const uint32_t* labels, int32_t nlabels,
                             int64_t row0 /* GLOBAL */, int64_t nrows,
                             const uint32_t* row_labels /* host, nrows, or NULL: the index's label column */,
                             double* out_sums /* (nlabels, d) C-contiguous, or NULL */,
                             int64_t* out_counts /* nlabels, or NULL */);

/* Diverse retrieval: maximal-marginal-relevance (MMR) re-ranking of the fetch_k best rows, on the device -- the answer
 * to "the top 10 are ten versions of one paragraph" in a corpus of chunked documents, overlapping windows and
 * near-copies.
 * Exact definition, per query q of the call:
 *   1. Candidates.  C = the list svs_index_search(idx, queries, nq, d, fetch_k, ...) returns for query q (this call's
 *      nq, coalescing off): c = min(fetch_k, live rows) entries in (score desc, row desc) order, s[p] the score bits
 *      of position p.  Every route of the ordinary search is taken unchanged; tombstoned rows never appear.
 *   2. Similarity.  G[i][j] = the dot product of the STORED values of candidate rows i and j (what
 *      svs_index_debug_dequant shows: f32 as is; f16 widened; fp8 as e4m3 x row scale), f32 products accumulated in
 *      f32 over the columns in ascending order as ONE fmaf chain per element; fp8 sums the e4m3 values and multiplies
 *      by (scale_i * scale_j) once, after the sum.  G[i][j] depends only on the two rows' stored values and on d --
 *      not on positions, c, nq or tiles -- and G[i][j] == G[j][i] bit for bit.
 *   3. Greedy pick.  Pick 0 is position 0.  For t >= 1: red[p] = max over earlier picks j of G[p][j],
 *      obj[p] = lambda_mult * s[p] - (1 - lambda_mult) * red[p] in f32 (the compiler may fuse it), and the pick is the
 *      unpicked p with the largest obj; an exact tie goes to the LOWER position (the better score, at equal score
 *      the higher row).
 *   4. Outputs.  *out_count = min(max(k, 0), c), the same for every query, written by every successful call.  At
 *      out_*[q*k + t], t < count, in PICK order: the row (row_offset + local), s of the pick (the search's bits) and
 *      red of the pick when it was chosen (-inf for pick 0, the max over nothing); out_redundancy may be NULL.
 *      Entries past the count are not touched.
 * It follows that lambda_mult == 1 returns the first count entries of C (rows, order and bits, for finite data), that
 * k == 1 or c == 1 returns C[0] and launches nothing beyond the search, and that no row appears twice.
 * Non-finite scores or stored values neither fault nor hang: the call still returns count distinct candidates; which
 * ones is unspecified.
 * Errors: everything is validated before anything is launched, and a failing call writes no output.  d != index d or
 * an empty index -> SVS_ERR_SHAPE.  SVS_ERR_INVALID: nq < 0; null queries with nq > 0; lambda_mult NaN or outside
 * [0, 1]; 0 < fetch_k < k; fetch_k <= 0 with k > 0; null out_scores, out_rows or out_count with work to do (nq > 0 and
 * k > 0).  fetch_k > SVS_DIVERSE_MAX_FETCH -> SVS_ERR_UNSUPPORTED.  k <= 0 or nq == 0 -> SVS_OK, count 0, nothing
 * launched.
 * Cost: the search at fetch_k, then per block of queries (as many as keep the c x c f32 matrices within 64 MiB) one
 * tiled f32-MFMA kernel (2 c^2 d FLOP per query over rows that sit in HBM) and one workgroup per query for the picks.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared; waits for pending staging
 * copies; never goes through the coalescer: all as svs_index_search_rows.
 * Out of scope: svs_multi / row-sharded corpora, a device-pointer variant, fetch_k above SVS_DIVERSE_MAX_FETCH, and
 * diversity ACROSS the queries of one call (every query is re-ranked on its own). */
#define SVS_DIVERSE_MAX_FETCH 1024
int32_t svs_index_search_diverse(svs_index* idx, const float* queries, int32_t nq, int32_t d,
                                 int32_t k, int32_t fetch_k, float lambda_mult,
                                 float* out_scores, int64_t* out_rows /* stride k */,
                                 float* out_redundancy /* stride k, or NULL */, int32_t* out_count);

/* ---- neighbours of STORED rows ("more like this", near-duplicates of one document, the kNN graph):
 *      replaces a loop of np.dot(M, M[i]) + get_top_k per row (src/svs/kb.py:1623, src/svs/util.py:190-203;
 *      0.24 s per row at 1M x 1536 by the reference's published figure).  The rows are already in HBM in the
 *      dtype the kernels read: nothing is pulled out, pushed back or filtered on the host.
 *   rows      GLOBAL rows (row_offset + local, like svs_index_mask_rows), any order, repeats allowed; each
 *             position is answered on its own.  A row outside [row_offset, row_offset + n) -> SVS_ERR_INVALID;
 *             a tombstoned source row -> SVS_ERR_INVALID (the message names it); nrows < 0 -> SVS_ERR_INVALID.
 *             Every argument is validated before anything is launched; a failing call writes no output.
 *   count   = min(max(k, 0), live rows - 1), the same for every position (a source row is live); *out_count is
 *             written in every successful case.  nrows == 0 or k <= 0 -> count 0, nothing launched.
 *   result    position i: the search of stored row rows[i], used as the query, over all live rows EXCEPT rows[i]
 *             itself, order (score desc, row desc), at out[i*k .. i*k+count); entries past count are not touched
 *             (as svs_index_search).  Only the row id is excluded, never a score: other rows with the same
 *             content (exact duplicates) stay in.
 * Exact definition.  Positions are processed in blocks of SVS_NEIGHBORS_BLOCK consecutive positions.  For a block
 * with source rows R: svs_index_search(idx, Q, |R|, d, count + 1) with Q = svs_index_debug_dequant of those rows
 * (coalescing off); in each query's list the entry whose row is the source row is removed, or, if it is absent, the
 * last entry.  Rows, order and score bits equal that.  (The top count + 1 of all rows, minus the source row if present
 * and otherwise truncated, IS the top count of the others -- also when the source row is not among them: a short row,
 * a zero row.)  The block is a normal search: every route is reached unchanged (screened and unscreened single query,
 * 16-query, tiled, phased, fused), and k + 1 > 256 simply falls off the fused path, as any search with k > 256 does.
 * Blocking; re-entrant on one handle; holds a reference and the geometry lock shared, like svs_index_search; waits for
 * pending staging copies; never goes through the coalescer (svs_index_set_coalesce does not affect it).
 * Out of scope: svs_multi (call it on the shard that holds the row: the neighbours are then that shard's), row-sharded
 * corpora in several processes, and a device-pointer variant. */
#define SVS_NEIGHBORS_BLOCK 1024
int32_t svs_index_neighbors(svs_index* idx, const int64_t* rows, int64_t nrows, int32_t k,
                            float* out_scores, int64_t* out_rows, int32_t* out_count);

/* ---- pairwise: replaces np.dot(M, M.T) + get_top_pairs of
 *      document_top_pairwise_scores, src/svs/kb.py:1642-1671, src/svs/util.py:206-233 --
 * The k best-scoring row PAIRS (i < j; diagonal and lower triangle ignored), ordered
 * (score desc, then i desc, then j desc -- the reference's flat upper-triangle index,
 * descending).  count = min(max(k,0), n(n-1)/2).  Up to n*n = 2^32 scores (65,536 rows) the
 * n x n matrix is materialised in HBM like the reference materialises it in RAM.  Beyond that
 * nothing of that size exists: the exact k-th best pair score of a prefix block bounds the
 * answer from below, the tiled MFMA GEMM runs with the i < j mask and that bound in its
 * epilogue, and only the surviving pairs are ordered (same order key, same result).  Needs rows
 * of whole 128-byte lines there; SVS_ERR_UNSUPPORTED if millions of pairs pass the bound
 * (near-duplicate documents en masse) or k needs a prefix block past 2^32 scores. */
int32_t svs_index_top_pairs(svs_index* idx, int32_t k, float* out_scores, int64_t* out_i, int64_t* out_j,
                            int32_t* out_count);

/* ---- one process, several GPUs: the `devices, ndev` form of the create/search pair (SURVEY.md
 *      8(b), 8(e)).  Replaces the same reference lines as svs_index_create / svs_index_search
 *      (src/svs/kb.py:875-876, :1623-1626, src/svs/util.py:190-203) for a KB process that owns a whole
 *      node: the (n, d) matrix is row-sharded, shard g = rows [g * ceil(n / ndev), ...) on devices[g]
 *      (a device may be listed more than once); a search runs on every shard at once (one worker
 *      thread per shard inside the library), each returns its local top-k with GLOBAL rows, and the
 *      calling thread merges them under the same total order -- scores, rows and order are those of
 *      ONE index over the whole matrix, for any ndev.  No RCCL: the exchange is ndev * k * 12 bytes
 *      of host memory.  Reference counted and re-entrant like svs_index. ------------------------- */
typedef struct svs_multi svs_multi;
int32_t svs_multi_create(const float* host_rows, int64_t n, int32_t d, int32_t store_dtype,
                         const int32_t* devices, int32_t ndev, svs_multi** out);
/* Same contract as svs_index_search (count = min(max(k, 0), live rows of ALL shards)). */
int32_t svs_multi_search(svs_multi* m, const float* queries, int32_t nq, int32_t d, int32_t k,
                         float* out_scores, int64_t* out_rows, int32_t* out_count);
int32_t svs_multi_retain(svs_multi* m);
int32_t svs_multi_release(svs_multi* m);
/* Shard count, total rows (masked ones included), dimension, masked rows; any pointer may be NULL. */
int32_t svs_multi_info(svs_multi* m, int32_t* ndev, int64_t* n, int32_t* d, int64_t* n_masked);
/* As svs_index_set_coalesce, in front of the shards: concurrent single-query svs_multi_search calls are
 * answered together by one batched search per shard. */
int32_t svs_multi_set_coalesce(svs_multi* m, int32_t enable);
int32_t svs_multi_coalesce_stats(svs_multi* m, int64_t* passes, int64_t* queries);
/* Shard g as an ordinary index handle (one more reference: release it with svs_index_release),
 * e.g. for svs_index_mask_rows / svs_index_info on the shard that holds a row. */
int32_t svs_multi_shard(svs_multi* m, int32_t g, svs_index** out);

/* ---- parity support (tests): what the index really holds -------------------- */
/* Rows [row0, row0 + nrows) exactly as stored, dequantised to f32 (nrows x d,
 * C-contiguous, host).  f32: the rows; f16: half-rounded; fp8: e4m3 * row scale. */
int32_t svs_index_debug_dequant(svs_index* idx, int64_t row0, int64_t nrows, float* out);
/* The query as the kernels of this index's dtype see it (f32: unchanged; f16:
 * half-rounded; fp8: quantised with its own scale and dequantised), d floats, host. */
int32_t svs_index_debug_query(svs_index* idx, const float* query, int32_t d, float* out);

/* ---- measurement --------------------------------------------------------- */
/* enable = N > 0: record HIP events around the score and select stages of every N-th
 * subsequent search on this handle and accumulate them (N = 1: every search; the three
 * event records cost ~10 us of stream time per timed search).  0: off. */
int32_t svs_index_set_timing(svs_index* idx, int32_t enable);
/* Waits for outstanding timed searches, returns the sums, and resets them. */
int32_t svs_index_get_timing(svs_index* idx, svs_timing_t* out);

/* Screened single-query search (f32 indexes whose rows are 512 .. 4096 elements, a multiple of 512, in HBM).
 * mode 1 (the default; SVS_AMD_SCREEN=0 in the environment makes 0 the default): the index keeps an IEEE-half
 * shadow of its rows (+50 % HBM, counted in hbm_bytes); a single query is scored against the shadow (half the
 * bytes), the rows that a proven error bound leaves in contention are re-scored from the f32 rows, and the
 * result -- rows, order, score bits -- is that of the unscreened search.  If HBM has no room for the shadow the
 * index works without it.  mode 0: frees the shadow; every search reads the f32 rows.  mode 1 again rebuilds it
 * from the rows in HBM.  Blocks searches on this handle while it runs. */
int32_t svs_index_set_screen(svs_index* idx, int32_t mode);

/* Tuning knob for A/B runs (bench/profiling only): selects a kernel variant of
 * the score stage; 0 = library default (11: never screen a single query, 12: screen
 * whatever the row count).  Returns SVS_ERR_INVALID if unknown. */
int32_t svs_index_set_variant(svs_index* idx, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* SVS_AMD_H */

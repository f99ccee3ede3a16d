"""
The seam between SVS's KB classes and the HIP backend.

``DeviceEmbeddingsMatrix`` has the surface of the reference's
``_EmbeddingsMatrix`` (src/svs/kb.py:856-893: ``get_sync`` / ``get`` /
``invalidate``) but what it caches is an HBM-resident ``DeviceIndex`` next to the
``emb_id_lookup`` array.  Two ways to put it under the reference's
``retrieve()``:

* the explicit 3-line patch of INTEGRATION.md (``superheavy()`` calls
  ``matrix.search(query_vec, n)``), or
* ``attach(kb)``: no reference line changes.  ``get_sync`` then returns a
  ``DeviceMatrixView`` in place of the numpy matrix; the reference's own
  ``np.dot(embeddings_matrix, query_vec)`` (kb.py:1623) and
  ``np.argpartition(scores, -top_k)`` (util.py:202) are routed to the device
  through NumPy's ``__array_function__`` protocol, and ``float(scores[i])``
  (util.py:203) reads the scores the device returned.  The reference's
  ``sorted(..., reverse=True)`` then orders them exactly as before.
"""
from __future__ import annotations

import asyncio
import logging
import threading
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

from .coalesce import SearchCoalescer
from .index import DeviceIndex

_LOG = logging.getLogger(__name__)

MatrixBuilder = Callable[[Any], Tuple[np.ndarray, np.ndarray]]


def _default_builder(db) -> Tuple[np.ndarray, np.ndarray]:
    """``with db as q: q.build_embeddings_matrix()`` -- the reference's own
    producer (src/svs/kb.py:872-873)."""
    with db as q:
        return q.build_embeddings_matrix()


class _Lookup:
    """Row -> embedding-id table of one NUMBERING of a loaded matrix.  ``arr`` only ever grows
    (append) and masked rows are never returned, so a search that started before an
    append can map its rows through the CURRENT array; a search that outlives an
    ``invalidate()`` keeps this object (and so the right table) alive.

    An in-place compaction (``DeviceEmbeddingsMatrix.remove``) renumbers the rows of the SAME index:
    it sets ``stale`` on this object before the rows move, never touches ``arr``, and installs a new
    ``_Lookup`` for the new numbering.  The index makes a compaction and a search exclude each other,
    so rows are in this object's numbering exactly when ``stale`` still reads False AFTER the native
    call that produced them (``search_mapped``)."""

    def __init__(self, arr: np.ndarray):
        self.arr = arr
        self.stale = False
        # positions of ``arr`` tombstoned in this numbering (``DeviceEmbeddingsMatrix.remove``), ascending; replaced, never
        # edited in place.  Only ``assign_op`` needs it: every search leaves masked rows out on the device.
        self.dead = np.zeros(0, dtype=np.int64)


def search_mapped(hold: Callable[[], tuple], held: tuple, native: Callable[..., Any], finish: Callable[[Any, np.ndarray], Any]):
    """Every search that maps rows through a lookup goes through here.  ``held`` = ``(idx, lookup, ...)`` as
    ``hold()`` / ``hold_search()`` returned it (the caller owns and releases that reference); ``native(*held)``
    runs the search and returns rows in the index's numbering; ``finish(result, lookup.arr)`` maps them to ids.

    The native call comes first, the read of ``lookup.stale`` second: False proves that no compaction had
    begun when the search ran, so its rows are in that lookup's numbering.  True: the rows may be in either
    numbering (and a search given rows of the old one may have failed on them); they are dropped, a fresh
    ``hold()`` -- released here -- is taken and the search repeated."""
    own = None
    try:
        while True:
            lookup = held[1]
            try:
                res = native(*held)
            except Exception:
                if not lookup.stale:
                    raise
                res = None
            if not lookup.stale:
                return finish(res, lookup.arr)   # (an append during the search only extends arr)
            if own is not None:
                own.release()
                own = None
            held = hold()
            own = held[0]
    finally:
        if own is not None:
            own.release()


def _within_rows(idx, lookup: _Lookup, emb_ids) -> np.ndarray:
    """GLOBAL rows of ``emb_ids`` in the numbering of ``lookup`` (strictly increasing ids: one ``searchsorted``,
    as ``remove`` does).  KeyError for an id the loaded matrix does not hold."""
    ids = np.asarray(emb_ids if isinstance(emb_ids, np.ndarray) else list(emb_ids), dtype=np.int64).reshape(-1)
    arr = lookup.arr
    pos = np.searchsorted(arr, ids)
    if len(ids):
        bad = pos >= len(arr)
        if len(arr):
            bad |= arr[np.minimum(pos, len(arr) - 1)] != ids
        if bad.any():
            raise KeyError(int(ids[np.argmax(bad)]))
    return pos + int(getattr(idx, "row_offset", 0))


# The mapped searches: each returns its (native, finish) pair for ``search_mapped`` -- ``native(idx, lookup[, co])`` maps
# embedding ids to rows of THAT lookup and runs the search, ``finish(result, lookup.arr)`` maps the rows back to ids.
# ``DeviceEmbeddingsMatrix.run_mapped`` runs one.

def single_op(query_vec: np.ndarray, n: int):
    """One query: [(score, emb_id)].  Through the generation's coalescer when ``hold_search`` gave one (concurrent
    callers -- threads of a server, AsyncKB's executor threads -- share corpus passes)."""
    def native(idx, lookup, co):
        return co.search(idx, query_vec, n) if co is not None else idx.search(query_vec, n)

    return native, ids_of_rows


def batch_op(query_vecs: np.ndarray, n: int):
    """``idx.search_batch``: one [(score, emb_id)] list per row of ``query_vecs``."""
    return (lambda idx, lookup: idx.search_batch(query_vecs, n)), ids_of_batch


def pairs_op(n: int):
    """``idx.top_pairs`` (svs_index_top_pairs): [(score, emb_id_1, emb_id_2)]."""
    return (lambda idx, lookup: idx.top_pairs(n)), ids_of_pairs


def within_op(query_vec: np.ndarray, n: int, emb_ids):
    """Top-n among ``emb_ids``: ids -> rows through ``lookup.arr``, the filtered search, rows -> ids.  KeyError for an
    id the loaded matrix does not hold."""
    def native(idx, lookup, *_):
        return idx, idx.search_within(query_vec, n, _within_rows(idx, lookup, emb_ids))

    def finish(res, arr):
        used, rows = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off])) for score, row in rows]

    return native, finish


def segments_op(query_vecs: np.ndarray, n: int, emb_id_lists, seg_query=None):
    """``within_op`` for many id lists in one native call (``idx.search_segments``, svs_index_search_segments): list s
    is searched with query ``seg_query[s]`` of ``query_vecs`` (None: query s).  One [(score, emb_id)] list per id list.
    KeyError for an id the loaded matrix does not hold."""
    id_lists = [e if isinstance(e, np.ndarray) else list(e) for e in emb_id_lists]

    def native(idx, lookup, *_):
        return idx, idx.search_segments(query_vecs, n, [_within_rows(idx, lookup, e) for e in id_lists], seg_query)

    def finish(res, arr):
        used, per_seg = res
        off = int(getattr(used, "row_offset", 0))
        return [list(zip(s.astype(np.float64).tolist(), arr[r - off].tolist())) for s, r in per_seg]

    return native, finish


def neighbors_op(emb_ids, n: int):
    """Neighbours of stored embeddings: ids -> rows through ``lookup.arr``, ``idx.neighbors`` (svs_index_neighbors),
    rows -> ids: one [(score, emb_id)] list per id, in the order given.  KeyError for an id the loaded matrix does not
    hold."""
    def native(idx, lookup, *_):
        return idx, idx.neighbors(_within_rows(idx, lookup, emb_ids), n)

    def finish(res, arr):
        used, (scores, rows) = res
        return ids_of_batch((scores, rows - int(getattr(used, "row_offset", 0))), arr)

    return native, finish


def above_op(query_vec: np.ndarray, min_score: float, n: int):
    """Threshold search: ``idx.search_above`` (svs_index_search_above), rows -> ids: ([(score, emb_id)], total)."""
    def native(idx, lookup, *_):
        return idx, idx.search_above(query_vec, min_score, n)

    def finish(res, arr):
        used, (rows, total) = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off])) for score, row in rows], int(total)

    return native, finish


def labeled_op(query_vec: np.ndarray, n: int, labels):
    """Labelled search: ``idx.search_labeled`` (svs_index_search_labeled) over the rows whose stored label is in
    ``labels``, rows -> ids: ([(score, emb_id)], rows that carry such a label).  The column is whatever the index holds
    (``DeviceEmbeddingsMatrix.ensure_labels``)."""
    def native(idx, lookup, *_):
        return idx, idx.search_labeled(query_vec, n, labels)

    def finish(res, arr):
        used, (rows, matched) = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off])) for score, row in rows], int(matched)

    return native, finish


def where_op(query_vec: np.ndarray, n: int, where):
    """Predicate search: ``idx.search_where`` (svs_index_search_where) over the rows on which every term of ``where``
    holds, rows -> ids: ([(score, emb_id)], rows that satisfy the predicate).  The columns are whatever the index holds
    (``DeviceEmbeddingsMatrix.ensure_column``)."""
    def native(idx, lookup, *_):
        return idx, idx.search_where(query_vec, n, where)

    def finish(res, arr):
        used, (rows, matched) = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off])) for score, row in rows], int(matched)

    return native, finish


def by_label_op(query_vec: np.ndarray, labels, min_score: Optional[float] = None, n: Optional[int] = None):
    """Per-label breakdown: ``idx.search_by_label`` (svs_index_search_by_label) over ``labels``, rows -> ids:
    [(label, score, emb_id of the label's best row, rows of the label at or above ``min_score``)], best label first.
    The column is whatever the index holds (``DeviceEmbeddingsMatrix.ensure_labels``)."""
    def native(idx, lookup, *_):
        return idx, idx.search_by_label(query_vec, labels, min_score, n)

    def finish(res, arr):
        used, groups = res
        off = int(getattr(used, "row_offset", 0))
        return [(int(label), score, int(arr[row - off]), int(total)) for label, score, row, total in groups]

    return native, finish


def collapsed_op(query_vec: np.ndarray, n: int, column: int, zero: str = "single"):
    """Collapsed search: ``idx.search_collapsed`` (svs_index_search_collapsed), at most one row per value of column
    ``column``, rows -> ids: ([(score, emb_id, value)], groups), best first.  The column is whatever the index holds
    (``DeviceEmbeddingsMatrix.ensure_column``)."""
    def native(idx, lookup, *_):
        return idx, idx.search_collapsed(query_vec, n, column, zero)

    def finish(res, arr):
        used, (rows, groups) = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off]), int(value)) for score, row, value in rows], int(groups)

    return native, finish


def _collapsed_scoped_finish(res, arr):
    """([(score, row, value)], groups, matched) of a scoped collapsed search, rows -> ids."""
    used, (rows, groups, matched) = res
    off = int(getattr(used, "row_offset", 0))
    return [(score, int(arr[row - off]), int(value)) for score, row, value in rows], int(groups), int(matched)


def collapsed_where_op(query_vec: np.ndarray, n: int, where, column: int, zero: str = "single"):
    """Collapsed search under a predicate: ``idx.search_collapsed_where`` (svs_index_search_collapsed_where), at most
    one row per value of column ``column`` among the rows on which every term of ``where`` holds, rows -> ids:
    ([(score, emb_id, value)], groups, rows that satisfy the predicate).  The columns are whatever the index holds
    (``DeviceEmbeddingsMatrix.ensure_column``)."""
    def native(idx, lookup, *_):
        return idx, idx.search_collapsed_where(query_vec, n, where, column, zero)

    return native, _collapsed_scoped_finish


def collapsed_within_op(query_vec: np.ndarray, n: int, emb_ids, column: int, zero: str = "single"):
    """Collapsed search over ``emb_ids``: ids -> rows through ``lookup.arr``, ``idx.search_collapsed_within``
    (svs_index_search_collapsed_rows), rows -> ids: ([(score, emb_id, value)], groups, live listed rows).  KeyError for
    an id the loaded matrix does not hold."""
    def native(idx, lookup, *_):
        return idx, idx.search_collapsed_within(query_vec, n, _within_rows(idx, lookup, emb_ids), column, zero)

    return native, _collapsed_scoped_finish


def collapsed_combined_op(vectors: np.ndarray, n: int, column: int, op: str = "max", weights=None, zero: str = "single"):
    """Group-combined search: ``idx.search_collapsed_combined`` (svs_index_search_collapsed_combined) of the (m, D)
    ``vectors`` over the groups of column ``column``, representative rows -> ids: ([(score, emb_id, value)], groups)."""
    def native(idx, lookup, *_):
        return idx, idx.search_collapsed_combined(vectors, n, column, op, weights, zero)

    def finish(res, arr):
        used, (rows, groups) = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off]), int(value)) for score, row, value in rows], int(groups)

    return native, finish


def diverse_op(query_vec: np.ndarray, n: int, fetch_k: Optional[int] = None, lam: float = 0.5):
    """Diverse (MMR) search: ``idx.search_diverse`` (svs_index_search_diverse), rows -> ids:
    [(score, emb_id, redundancy)] in pick order."""
    def native(idx, lookup, *_):
        return idx, idx.search_diverse(query_vec, n, fetch_k, lam)

    def finish(res, arr):
        used, rows = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off]), red) for score, row, red in rows]

    return native, finish


def combined_op(vectors: np.ndarray, n: int, op: str = "max", weights=None):
    """Combined search: ``idx.search_combined`` (svs_index_search_combined) of the (m, D) ``vectors``, rows -> ids:
    [(score, emb_id)]."""
    def native(idx, lookup, *_):
        return idx, idx.search_combined(vectors, n, op, weights)

    def finish(res, arr):
        used, rows = res
        off = int(getattr(used, "row_offset", 0))
        return [(score, int(arr[row - off])) for score, row in rows]

    return native, finish


def assign_op(vectors: np.ndarray):
    """Nearest-vector assignment of every LIVE stored embedding: ``idx.assign`` (svs_index_assign) over the whole index
    without touching the label column, rows -> ids: (emb_ids i64 (m,), best i32 (m,), scores f32 (m,), counts i64 (c,))
    in row order.  The tombstoned rows are dropped here (the device answers for them too)."""
    def native(idx, lookup, *_):
        dead = lookup.dead          # (before the call: a removal that lands during it may or may not be in the counts)
        return dead, idx.assign(vectors)

    def finish(res, arr):
        dead, (best, scores, counts) = res
        live = np.ones(len(best), dtype=bool)
        live[dead[dead < len(best)]] = False
        ids = np.asarray(arr[:len(best)], dtype=np.int64)[live]
        best = best[live]
        if int(counts.sum()) != len(best):   # a removal landed between the read of ``dead`` and the device's bitmap
            counts = np.bincount(best, minlength=len(counts)).astype(np.int64)
        return ids, best, scores[live], counts

    return native, finish


def cluster_op(c: int, iterations: int = 10, seed: int = 0):
    """k-means over every stored embedding: ``idx.kmeans`` (svs_index_assign + svs_index_label_sums per iteration)
    without touching the label column, rows -> ids: (emb_ids i64 (m,), cluster i32 (m,), scores f32 (m,), counts i64
    (c,), centroids f32 (c, D), iterations run) in row order, tombstoned rows dropped as in ``assign_op``.  The WHOLE loop
    is one mapped op: a compaction that lands inside it fails or stales the op as a whole, and ``search_mapped`` runs
    it again -- never two iterations in two numberings."""
    def native(idx, lookup, *_):
        dead = lookup.dead
        return dead, idx.kmeans(c, iterations, seed)

    def finish(res, arr):
        dead, (centroids, best, scores, counts, ran) = res
        live = np.ones(len(best), dtype=bool)
        live[dead[dead < len(best)]] = False
        ids = np.asarray(arr[:len(best)], dtype=np.int64)[live]
        best = best[live]
        if int(counts.sum()) != len(best):   # a removal landed between the read of ``dead`` and the device's bitmap
            counts = np.bincount(best, minlength=len(counts)).astype(np.int64)
        return ids, best, scores[live], counts, centroids, ran

    return native, finish


def ids_of_rows(res, arr: np.ndarray) -> List[Tuple[float, int]]:
    return [(score, int(arr[row])) for score, row in res]


def ids_of_batch(res, arr: np.ndarray) -> List[List[Tuple[float, int]]]:
    scores, rows = res
    ids = arr[rows]                                   # (one gather for the whole batch)
    sc = scores.astype(np.float64)
    return [list(zip(sc[i].tolist(), ids[i].tolist())) for i in range(len(scores))]


def ids_of_pairs(res, arr: np.ndarray) -> List[Tuple[float, int, int]]:
    return [(score, int(arr[i]), int(arr[j])) for score, i, j in res]


class DeviceEmbeddingsMatrix:
    """Lazy cache of (DeviceIndex, emb_id_lookup); drop-in for
    ``svs.kb._EmbeddingsMatrix``."""

    # reclaim the dead rows (compaction in place, or a rebuild from storage) once this share of the rows is dead
    COMPACT_AT = 0.25

    def __init__(self, device: int = 0, builder: MatrixBuilder = _default_builder,
                 index_factory: Callable[..., Any] = DeviceIndex, keep_host_matrix: bool = True,
                 view: bool = False, block_builder: Optional[Callable[[Any], Any]] = None):
        self.device = device
        self._builder = builder
        # optional streaming producer: db -> iterator of (n, m), then (ids, rows) blocks
        # (svs_amd.kb._blocks_from_store); used when no host copy is kept and the index type can
        # start empty and grow (DeviceIndex.empty / append)
        self._block_builder = block_builder
        self._index_factory = index_factory
        self._keep_host = keep_host_matrix
        self._view = view
        self._mu = threading.Lock()
        self.index: Optional[Any] = None
        self.embeddings_matrix: Optional[np.ndarray] = None   # host copy (pairwise path), optional
        self._lookup: Optional[_Lookup] = None
        self._n_dead = 0
        # column -> the index generation for which it is installed and complete (ensure_column); absent: none is.
        # Column 0 is the label column (ensure_labels).
        self._columns_for: Dict[int, Any] = {}
        # concurrent single-query searches of one index generation share corpus passes (coalesce.py)
        self.coalesce = True
        self._coalescer: Optional[SearchCoalescer] = None

    @property
    def emb_id_lookup(self) -> Optional[np.ndarray]:
        lk = self._lookup
        return lk.arr if lk is not None else None

    # -- reference surface ------------------------------------------------
    def invalidate(self) -> None:
        """src/svs/kb.py:861-864.  In-flight searches keep the HBM copy alive
        (the handle is reference counted)."""
        _LOG.info("invalidating cached vectors; they'll be re-built next time you `retrieve()`")
        with self._mu:
            idx, self.index = self.index, None
            self.embeddings_matrix = None
            self._lookup = None
            self._n_dead = 0
            self._columns_for = {}
            self._coalescer = None
        if idx is not None:
            idx.release()

    def _empty_factory(self):
        """(d, reserve) -> an empty index of the configured type, or None if the type cannot grow
        from nothing (test doubles, MultiDeviceIndex)."""
        f, kw = self._index_factory, {}
        if hasattr(f, "func") and hasattr(f, "keywords"):     # functools.partial(DeviceIndex, dtype=...)
            f, kw = f.func, dict(f.keywords)
        make = getattr(f, "empty", None)
        if make is None:
            return None
        return lambda d, reserve: make(d, device=self.device, reserve=reserve, **kw)

    def _build_and_install(self, db):
        """Cold start (src/svs/kb.py:573-618 + :875-876).  Streaming when possible: BLOB -> 32 MiB
        block -> svs_index_append (pinned staging, DMA overlapped with the next block's copy) -- the
        reference's (n, m) host matrix is never materialised; otherwise matrix-then-upload."""
        make = self._empty_factory() if (self._block_builder is not None and not self._keep_host) else None
        if make is None:
            matrix, lookup = self._builder(db)
            return self._install(matrix, lookup)
        holder: dict = {}
        # blocks are decoded straight into the library's pinned staging memory when the index offers it
        acquire = (lambda: holder["idx"].staging_acquire()) if hasattr(getattr(self._index_factory, "func", self._index_factory),
                                                                        "staging_acquire") else None
        try:
            blocks = self._block_builder(db, acquire=acquire)
        except TypeError:            # a block builder without the `acquire` hook
            acquire = None
            blocks = self._block_builder(db)
        n, m = next(blocks)
        if n * m == 0:
            for _ in blocks:
                pass
            return self._install(np.zeros((n, m), dtype=np.float32), np.zeros(n, dtype=np.int64))
        idx = holder["idx"] = make(m, n)
        ids_all = np.empty(n, dtype=np.int64)
        fill = 0
        try:
            for ids, rows in blocks:
                if acquire is not None:
                    idx.staging_commit(len(ids))      # DMA enqueued; the next block is decoded meanwhile
                else:
                    idx.append(rows)                  # copies out of the reused block before returning
                ids_all[fill:fill + len(ids)] = ids
                fill += len(ids)
            if acquire is not None:
                idx.staging_finish()
            assert fill == n and idx.shape == (n, m)
        except BaseException:
            idx.release()
            raise
        self._apply_coalesce(idx)
        with self._mu:
            self.index = idx
            self._lookup = _Lookup(ids_all)
            self._n_dead = 0
            self.embeddings_matrix = None
        return idx

    def _apply_coalesce(self, idx) -> None:
        """Switch the library's coalescing on for a freshly built index (so that the zero-diff
        ``attach()`` path, which reaches the index through np.dot / np.argpartition, gets it too)."""
        if hasattr(idx, "set_coalesce"):
            idx.set_coalesce(bool(self.coalesce))
            idx._coalesce_applied = bool(self.coalesce)

    def _install(self, matrix: np.ndarray, lookup: np.ndarray):
        idx = self._index_factory(matrix, device=self.device)
        self._apply_coalesce(idx)
        with self._mu:
            self.index = idx
            self._lookup = _Lookup(lookup)
            self._n_dead = 0
            self.embeddings_matrix = matrix if self._keep_host else None
        return idx

    # -- incremental update ---------------------------------
    def append(self, new_rows: np.ndarray, new_ids, labels=None, columns: Optional[Dict[int, Any]] = None) -> bool:
        """Rows a ``bulk_add_docs`` just committed, in embedding-id order (the order
        ``SELECT id, embedding FROM embeddings`` would return them, src/svs/kb.py:603).
        Edits the HBM copy in place; False if nothing is loaded (the next ``get``
        builds from storage anyway).  ``columns``: {column: one value per new row}, each set behind the append while
        this generation's column is installed (``ensure_column``); an append WITHOUT values for an installed column
        marks it not installed -- the new rows carry 0 there until the next ``ensure_column`` installs the whole column
        again.  ``labels`` is ``columns[0]``."""
        given = dict(columns or {})
        if labels is not None:
            given[0] = labels
        new_rows = np.ascontiguousarray(new_rows, dtype=np.float32)
        ids = np.asarray(new_ids, dtype=np.int64)
        with self._mu:
            idx, lk = self.index, self._lookup
            if idx is None or lk is None:
                return False
            if len(ids) == 0:
                return True
            if new_rows.ndim != 2 or new_rows.shape[0] != len(ids) or (len(lk.arr) and ids[0] <= lk.arr[-1]) \
                    or np.any(np.diff(ids) <= 0) or new_rows.shape[1] != idx.shape[1]:
                idx = None   # not a pure append (or dimension change): rebuild
            else:
                installed = [c for c, gen in self._columns_for.items() if gen is idx]
                self._columns_for = {}       # (until the new rows' values are in: a failure below leaves it so)
                row0 = int(getattr(idx, "row_offset", 0)) + len(lk.arr)
                idx.append(new_rows)
                lk.arr = np.concatenate([lk.arr, ids])
                for c in installed:
                    values = given.get(c)
                    if values is None:
                        continue
                    if len(values) != len(ids):
                        raise ValueError(f"{len(values)} {'labels' if c == 0 else f'values of column {c}'} for {len(ids)} new rows")
                    self._set_column(idx, c, values, row0)
                    self._columns_for[c] = idx
                if self.embeddings_matrix is not None:
                    self.embeddings_matrix = np.vstack([self.embeddings_matrix, new_rows])
        if idx is None:
            self.invalidate()
            return False
        return True

    def remove(self, emb_ids) -> bool:
        """Embeddings a ``bulk_del_docs`` just committed: their rows are tombstoned in
        HBM (never returned again, other rows keep their indices).  Once ``COMPACT_AT`` of the rows
        are dead they are reclaimed: in place on the device when the index can (``compact``), no host
        copy is kept and no ``attach()`` view has handed the lookup array out -- the index object stays,
        nothing is read from storage -- and by a rebuild from storage otherwise."""
        ids = np.asarray(list(emb_ids), dtype=np.int64)
        rebuild = False
        with self._mu:
            idx, lk = self.index, self._lookup
            if idx is None or lk is None:
                return False
            if len(ids) == 0:
                return True
            pos = np.searchsorted(lk.arr, ids)
            if np.any(pos >= len(lk.arr)) or np.any(lk.arr[np.minimum(pos, len(lk.arr) - 1)] != ids):
                rebuild = True
            else:
                self._n_dead += len(ids)
                off = int(getattr(idx, "row_offset", 0))
                if self.embeddings_matrix is not None:
                    rebuild = True      # a host copy would go stale: rebuild from storage
                elif self._n_dead <= self.COMPACT_AT * len(lk.arr):
                    idx.mask_rows(pos + off)
                    lk.dead = np.union1d(lk.dead, pos)
                elif self._view or not hasattr(idx, "compact"):
                    rebuild = True      # compaction by a rebuild from storage
                else:
                    # searches that hold (idx, lk) read the flag AFTER their native call (search_mapped): set
                    # before the first row moves, and lk.arr stays as it is
                    lk.stale = True
                    try:
                        idx.mask_rows(pos + off)
                        old_rows = idx.compact()
                        self._lookup = _Lookup(lk.arr[np.asarray(old_rows, dtype=np.int64) - off])
                        self._n_dead = 0
                    except Exception:  # noqa: BLE001 -- e.g. a device error half way: the rows are in no defined order
                        _LOG.exception("in-place compaction failed; the cached vectors will be re-built")
                        rebuild = True
        if rebuild:
            self.invalidate()
            return False
        return True

    def _result(self):
        m = DeviceMatrixView(self.index, self.embeddings_matrix) if self._view else self.embeddings_matrix
        return m, self.emb_id_lookup

    def get_sync(self, db) -> Tuple[Any, np.ndarray]:
        """src/svs/kb.py:866-877."""
        if self.index is not None and self._lookup is not None:
            _LOG.info("using cached vectors")
            return self._result()
        _LOG.info("re-building cached vectors...")
        self._build_and_install(db)
        _LOG.info("re-building cached vectors... DONE!")
        return self._result()

    async def get(self, db) -> Tuple[Any, np.ndarray]:
        """src/svs/kb.py:879-893 (the build runs on an executor thread)."""
        if self.index is not None and self._lookup is not None:
            _LOG.info("using cached vectors")
            return self._result()
        _LOG.info("re-building cached vectors...")
        loop = asyncio.get_running_loop()
        await loop.run_in_executor(None, lambda: self._build_and_install(db))
        _LOG.info("re-building cached vectors... DONE!")
        return self._result()

    # -- the superheavy() body ---------------------------------------------
    def run_mapped(self, op, held: Optional[tuple] = None, single: bool = False):
        """Runs one mapped search (``single_op`` ... ``above_op``) through ``search_mapped``.  ``held``: the caller's own
        ``hold()`` -- ``hold_search()`` for ``single`` -- which the caller releases; None: one is taken and released
        here.  Either way the fresh holds of a retry after a compaction come from the same source and are released by
        ``search_mapped``."""
        hold = self.hold_search if single else self.hold
        if held is not None:
            return search_mapped(hold, held, *op)
        held = hold()
        try:
            return search_mapped(hold, held, *op)
        finally:
            held[0].release()

    def search(self, query_vec: np.ndarray, n: int) -> List[Tuple[float, int]]:
        """``superheavy()`` (src/svs/kb.py:1622-1627): [(score, emb_id)]."""
        return self.run_mapped(single_op(query_vec, n), single=True)

    def search_within(self, query_vec: np.ndarray, n: int, emb_ids) -> List[Tuple[float, int]]:
        """``search`` restricted to the listed embedding ids: [(score, emb_id)] (``KB.retrieve_within``)."""
        return self.run_mapped(within_op(query_vec, n, emb_ids))

    def search_above(self, query_vec: np.ndarray, min_score: float, n: int) -> Tuple[List[Tuple[float, int]], int]:
        """Every stored embedding scoring at or above ``min_score``, best first, at most ``n``:
        ([(score, emb_id)], total qualifying) (``KB.retrieve_above``)."""
        return self.run_mapped(above_op(query_vec, min_score, n))

    @staticmethod
    def _set_column(idx, c: int, values, row0=None) -> None:
        """Column 0 goes through ``set_labels``: it is the label column, and every index double has that entry."""
        if c == 0:
            idx.set_labels(values, row0)
        else:
            idx.set_column(c, values, row0)

    def ensure_labels(self, fetch: Callable[[], Tuple[Any, Any]]) -> bool:
        """``ensure_column(0, fetch)``: the label column."""
        return self.ensure_column(0, fetch)

    def ensure_column(self, c: int, fetch: Callable[[], Tuple[Any, Any]]) -> bool:
        """Column ``c`` of the loaded index generation, installed at most once per generation: a no-op (False) while
        it is installed; otherwise ``fetch()`` -> (embedding ids, values), any order, is mapped to rows with one
        ``searchsorted`` on the lookup, rows nobody names get 0, and ONE write sets the whole range (True).
        Ids the loaded matrix does not hold (committed, not yet appended) are skipped: their ``append`` brings their
        values.  ``append`` and this method exclude each other, so a row is never left with a stale value: it is
        written by whichever of the two saw it last."""
        with self._mu:
            idx, lk = self._loaded()
            if self._columns_for.get(c) is idx:
                return False
            ids, labels = fetch()
            ids = np.asarray(ids, dtype=np.int64).reshape(-1)
            labels = np.asarray(labels, dtype=np.uint32).reshape(-1)
            arr = lk.arr
            column = np.zeros(len(arr), dtype=np.uint32)
            if len(arr) and len(ids):
                pos = np.minimum(np.searchsorted(arr, ids), len(arr) - 1)
                known = arr[pos] == ids
                column[pos[known]] = labels[known]
            if len(column):
                self._set_column(idx, c, column)
            self._columns_for[c] = idx
            return True

    def search_labeled(self, query_vec: np.ndarray, n: int, labels) -> Tuple[List[Tuple[float, int]], int]:
        """``search`` over the stored embeddings whose label is in ``labels``: ([(score, emb_id)], how many carry
        such a label) (``KB.retrieve_at_level``).  Call ``ensure_labels`` first."""
        return self.run_mapped(labeled_op(query_vec, n, labels))

    def search_where(self, query_vec: np.ndarray, n: int, where) -> Tuple[List[Tuple[float, int]], int]:
        """``search`` over the stored embeddings on which every term of ``where`` holds: ([(score, emb_id)], how many
        satisfy it) (``KB.retrieve_under``).  Call ``ensure_column`` for the columns it names first."""
        return self.run_mapped(where_op(query_vec, n, where))

    def search_by_label(self, query_vec: np.ndarray, labels, min_score: Optional[float] = None,
                        n: Optional[int] = None) -> List[Tuple[int, float, int, int]]:
        """The breakdown of one query over ``labels``: [(label, score, emb_id of the label's best embedding, how many
        of the label score at or above ``min_score``)], best label first (``KB.retrieve_by_level``).  Call
        ``ensure_labels`` first."""
        return self.run_mapped(by_label_op(query_vec, labels, min_score, n))

    def search_collapsed(self, query_vec: np.ndarray, n: int, column: int,
                         zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int]:
        """``search`` with at most one stored embedding per value of column ``column``, every value represented by its
        best one: ([(score, emb_id, value)], how many values -- and, with ``zero="single"``, value-0 embeddings -- have
        a live embedding) (``KB.retrieve_collapsed``).  Call ``ensure_column`` for the column first."""
        return self.run_mapped(collapsed_op(query_vec, n, column, zero))

    def search_collapsed_where(self, query_vec: np.ndarray, n: int, where, column: int,
                               zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int, int]:
        """``search_collapsed`` among the stored embeddings on which every term of ``where`` holds: ([(score, emb_id,
        value)], groups, how many satisfy the predicate) (``KB.retrieve_collapsed`` with levels).  Call
        ``ensure_column`` for every column named first."""
        return self.run_mapped(collapsed_where_op(query_vec, n, where, column, zero))

    def search_collapsed_within(self, query_vec: np.ndarray, n: int, emb_ids, column: int,
                                zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int, int]:
        """``search_collapsed`` among the listed embedding ids: ([(score, emb_id, value)], groups, live listed
        embeddings).  Call ``ensure_column`` for the column first."""
        return self.run_mapped(collapsed_within_op(query_vec, n, emb_ids, column, zero))

    def search_diverse(self, query_vec: np.ndarray, n: int, fetch_k: Optional[int] = None,
                       lam: float = 0.5) -> List[Tuple[float, int, float]]:
        """``search`` re-ranked for diversity (MMR over the ``fetch_k`` best, on the device):
        [(score, emb_id, redundancy)] in pick order (``KB.retrieve_diverse``)."""
        return self.run_mapped(diverse_op(query_vec, n, fetch_k, lam))

    def search_collapsed_combined(self, vectors: np.ndarray, n: int, column: int, op: str = "max", weights=None,
                                  zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int]:
        """``search_collapsed`` against several vectors at once (``DeviceIndex.search_collapsed_combined``: a group's
        score against each vector is its best row's, the m of them combined by ``op``): ([(score, emb_id of the
        group's representative, value)], groups) (``KB.retrieve_collapsed_combined``).  Call ``ensure_column`` first."""
        return self.run_mapped(collapsed_combined_op(vectors, n, column, op, weights, zero))

    def search_combined(self, vectors: np.ndarray, n: int, op: str = "max", weights=None) -> List[Tuple[float, int]]:
        """``search`` ranked against several vectors at once (``DeviceIndex.search_combined``: the "max", "min" or weighted
        "sum" of a row's scores against the (m, D) ``vectors``): [(score, emb_id)] (``KB.retrieve_combined``)."""
        return self.run_mapped(combined_op(vectors, n, op, weights))

    def assign(self, vectors: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """For every LIVE stored embedding, in row order, the row of ``vectors`` (c, D) it scores best against:
        (emb_ids i64 (m,), best i32 (m,), scores f32 (m,), counts i64 (c,)) (``KB.classify_documents``).  The label
        column is never written: on a KB it belongs to the levels (``ensure_labels``)."""
        return self.run_mapped(assign_op(vectors))

    def cluster(self, c: int, iterations: int = 10, seed: int = 0):
        """k-means of the stored embeddings into ``c`` clusters, on the device: (emb_ids i64 (m,), cluster i32 (m,),
        scores f32 (m,), counts i64 (c,), centroids f32 (c, D), iterations run) for the LIVE embeddings in row order
        (``KB.cluster_documents``).  The label column is never written."""
        return self.run_mapped(cluster_op(c, iterations, seed))

    def search_within_many(self, query_vecs: np.ndarray, n: int, emb_id_lists, seg_query=None) -> List[List[Tuple[float, int]]]:
        """``search_within`` for many id lists in one call: list s against query ``seg_query[s]`` of ``query_vecs``
        (None: query s).  One [(score, emb_id)] list per id list (``KB.retrieve_many_within`` /
        ``KB.retrieve_within_each``)."""
        return self.run_mapped(segments_op(query_vecs, n, emb_id_lists, seg_query))

    def search_many(self, query_vecs: np.ndarray, n: int) -> List[List[Tuple[float, int]]]:
        """Batched ``superheavy()``: one result list per row of ``query_vecs``;
        up to 16 (f32) / 32 (f16) queries share one pass over the corpus."""
        return self.run_mapped(batch_op(query_vecs, n))

    def neighbors(self, emb_ids, n: int) -> List[List[Tuple[float, int]]]:
        """The ``n`` nearest stored embeddings of each listed embedding id, itself excluded: one
        [(score, emb_id)] list per id, in the order given (``KB.retrieve_similar`` / ``document_neighbors``).
        KeyError for an id the loaded matrix does not hold."""
        return self.run_mapped(neighbors_op(emb_ids, n))

    def top_pairs(self, n: int) -> List[Tuple[float, int, int]]:
        """``superheavy()`` of document_top_pairwise_scores (src/svs/kb.py:1650-1655):
        [(score, emb_id_1, emb_id_2)]."""
        return self.run_mapped(pairs_op(n))

    def _loaded(self) -> Tuple[Any, _Lookup]:
        """(index, lookup) of the loaded matrix, no reference taken; call it under ``_mu``."""
        idx, lookup = self.index, self._lookup
        if idx is None or lookup is None:
            raise RuntimeError("embeddings matrix is not loaded (call get_sync/get first)")
        return idx, lookup

    def hold(self) -> Tuple[Any, _Lookup]:
        """(index, lookup table) with the caller owning a reference to the index, so a
        concurrent ``invalidate()`` cannot free it mid-search.  Map rows through
        ``lookup.arr`` AFTER the search returns; release the index."""
        with self._mu:
            idx, lookup = self._loaded()
            return idx.share(), lookup

    def hold_search(self) -> Tuple[Any, _Lookup, Optional[SearchCoalescer]]:
        """``hold()`` plus the generation's coalescer (None when switched off): what ``retrieve``
        uses for its single-query search."""
        with self._mu:
            idx, lookup = self._loaded()
            if hasattr(idx, "set_coalesce"):
                # a DeviceIndex coalesces inside the library (svs_index_set_coalesce): the waiting threads
                # block in C, without the GIL -- 64 callers: 20 k queries/s where the Python class below gets 12.6 k
                if getattr(idx, "_coalesce_applied", None) != bool(self.coalesce):
                    idx.set_coalesce(bool(self.coalesce))
                    idx._coalesce_applied = bool(self.coalesce)
                return idx.share(), lookup, None
            if self.coalesce and self._coalescer is None:
                self._coalescer = SearchCoalescer()
            return idx.share(), lookup, (self._coalescer if self.coalesce else None)


# --------------------------------------------------------------------------
# zero-diff attachment through NumPy's __array_function__ protocol
# --------------------------------------------------------------------------
class DeviceScores:
    """What ``np.dot(DeviceMatrixView, q)`` returns: a lazy length-N score
    vector.  ``np.argpartition(self, -k)`` runs the device search."""

    ndim = 1

    def __init__(self, index, query_vec: np.ndarray):
        self._index = index
        self._q = np.asarray(query_vec, dtype=np.float32)
        self._found = {}
        self.shape = (len(index),)
        self.dtype = np.dtype(np.float32)

    def __len__(self) -> int:
        return self.shape[0]

    def __getitem__(self, i):
        i = int(i)
        if i not in self._found:  # not produced by the last search: fetch the full vector once
            full = self._index.scores(self._q)
            self._found = {j: float(v) for j, v in enumerate(full)}
        return np.float32(self._found[i])

    def __array__(self, dtype=None, copy=None):
        out = self._index.scores(self._q)
        return out if dtype is None else out.astype(dtype)

    def __array_function__(self, func, types, args, kwargs):
        if func is np.argpartition and len(args) >= 2 and args[0] is self and not kwargs:
            kth = int(args[1])
            n = self.shape[0]
            if kth < 0 and -kth <= n:
                k = -kth
                res = self._index.search(self._q, k)
                self._found = {row: score for score, row in res}
                rows = np.fromiter((row for _, row in res), dtype=np.int64, count=len(res))
                # argpartition contract: the k largest occupy the last k slots
                out = np.empty(n, dtype=np.int64) if n == k else None
                if out is not None:
                    out[:] = rows[::-1]
                    return out
                return _TailOnly(rows[::-1], n)
        return func(*[np.asarray(a) if isinstance(a, DeviceScores) else a for a in args], **kwargs)


class _TailOnly:
    """Index vector of which only the last k entries are materialised (the only
    ones ``get_top_k`` reads: ``indices[-top_k:]``, src/svs/util.py:202)."""

    def __init__(self, tail: np.ndarray, n: int):
        self._tail, self._n = tail, n

    def __getitem__(self, sl):
        if isinstance(sl, slice) and sl.stop is None and sl.step is None and sl.start is not None \
                and sl.start < 0 and -sl.start <= len(self._tail):
            return self._tail[sl.start:]
        raise IndexError("only the top-k tail of a device argpartition is available")

    def __len__(self) -> int:
        return self._n


class DeviceMatrixView:
    """Stands in for the numpy ``embeddings_matrix`` inside the reference's
    ``retrieve()``.  ``.shape`` serves the log line (kb.py:1629); ``np.dot`` with
    a 1-D query goes to the device; anything else falls back to the host copy
    (e.g. ``np.dot(M, M.T)`` of document_top_pairwise_scores, kb.py:1651)."""

    def __init__(self, index, host_matrix: Optional[np.ndarray]):
        self._index = index
        self._host = host_matrix
        self.shape = tuple(index.shape)
        self.ndim = 2
        self.dtype = np.dtype(np.float32)

    def __len__(self) -> int:
        return self.shape[0]

    @property
    def T(self):
        return self._require_host().T

    def _require_host(self) -> np.ndarray:
        if self._host is None:
            raise RuntimeError("host copy of the embeddings matrix was not kept (keep_host_matrix=False)")
        return self._host

    def __array__(self, dtype=None, copy=None):
        h = self._require_host()
        return h if dtype is None else h.astype(dtype)

    def __array_function__(self, func, types, args, kwargs):
        if func is np.dot and len(args) == 2 and args[0] is self and not kwargs:
            q = np.asarray(args[1])
            if q.ndim == 1:
                if q.shape[0] != self.shape[1] or self.shape[0] == 0:
                    raise ValueError(f"shapes {self.shape} and {q.shape} not aligned: "
                                     f"{self.shape[1]} (dim 1) != {q.shape[0]} (dim 0)")
                return DeviceScores(self._index, q)
        return func(*[np.asarray(a) if isinstance(a, DeviceMatrixView) else a for a in args], **kwargs)


def attach(kb, device: int = 0, keep_host_matrix: bool = True, index_factory: Callable[..., Any] = DeviceIndex,
           devices: Optional[List[int]] = None, dtype: str = "f32"):
    """Swap a reference ``svs.KB`` / ``svs.AsyncKB`` instance's matrix cache for
    the device-backed one.  No reference source line changes; ``retrieve()``
    keeps its exact surface.  ``devices=[0, 1, ...]`` row-shards the corpus over
    several GPUs of this process (``svs_amd.multi.MultiDeviceIndex``); ``dtype``
    ("f32" = the reference's arithmetic, "f16", "fp8") is how the corpus is stored in HBM."""
    import functools
    if devices is not None and len(devices) > 1:
        from .multi import MultiDeviceIndex
        index_factory = functools.partial(MultiDeviceIndex, devices=list(devices), dtype=dtype)
    elif dtype != "f32":
        index_factory = functools.partial(index_factory, dtype=dtype)
    old = kb.embeddings_matrix
    new = DeviceEmbeddingsMatrix(device=device, keep_host_matrix=keep_host_matrix,
                                 index_factory=index_factory, view=True)
    kb.embeddings_matrix = new
    try:
        old.invalidate()
    except Exception:  # noqa: BLE001
        pass
    return kb

"""
DeviceIndex: the HBM-resident embedding matrix plus the fused
``np.dot(M, q)`` + ``get_top_k`` search of the reference's ``superheavy()``
closure (reference src/svs/kb.py:1622-1627 / :1184-1189, src/svs/util.py:190-203).

Thin host mirror over the C ABI (include/svs_amd.h).  All arithmetic happens in
the HIP kernels; this module only marshals numpy buffers.
"""
from __future__ import annotations

import ctypes as C
import operator
import threading
from typing import List, Optional, Tuple

import numpy as np

from . import _native


# HBM element type of the corpus.  "f32" is the reference layout; "f16" rounds
# rows (and queries) to half, f32 accumulate -- BASELINE.json configs[2]/[3];
# "fp8" stores OCP e4m3 with one f32 scale per row -- configs[4].
_DTYPES = {"f32": _native.DTYPE_F32, "f16": _native.DTYPE_F16, "fp8": _native.DTYPE_FP8}

DIVERSE_MAX_FETCH = 1024   # SVS_DIVERSE_MAX_FETCH: the most candidates (and so results) of a diverse search
LABELS_MAX_SET = 1024      # SVS_LABELS_MAX_SET: the most distinct labels one labelled search names
ASSIGN_MAX_VECTORS = 1024  # SVS_ASSIGN_MAX_VECTORS: the most vectors one assignment takes
COMBINE_MAX_VECTORS = _native.COMBINE_MAX_VECTORS   # SVS_COMBINE_MAX_VECTORS: the most vectors of one combined query
COMBINE_OPS = {"max": _native.COMBINE_MAX, "min": _native.COMBINE_MIN, "sum": _native.COMBINE_SUM}


def labels_u32(labels) -> np.ndarray:
    """Row labels, or the label set of a search, as a C-contiguous u32 vector; ValueError for a value outside
    [0, 2**32) or one that is no integer (a cast would silently name another label)."""
    a = np.asarray(labels if isinstance(labels, np.ndarray) else list(labels))
    if a.dtype != np.uint32:
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"labels must be integers, got dtype {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("labels must lie in [0, 2**32)")
        a = a.astype(np.uint32)
    return np.ascontiguousarray(a).reshape(-1)


COLUMNS_MAX = _native.COLUMNS_MAX          # SVS_COLUMNS_MAX: column 0 is the label column
WHERE_MAX_TERMS = _native.WHERE_MAX_TERMS  # SVS_WHERE_MAX_TERMS: the most terms of one predicate

# op name of a ``where`` term -> (svs_where_op, negate)
WHERE_OPS = {
    "in": (_native.WHERE_IN, 0), "not in": (_native.WHERE_IN, 1),
    "range": (_native.WHERE_RANGE, 0), "not range": (_native.WHERE_RANGE, 1),
    "any_bits": (_native.WHERE_ANY_BITS, 0), "no_bits": (_native.WHERE_ANY_BITS, 1),
    "all_bits": (_native.WHERE_ALL_BITS, 0), "not all_bits": (_native.WHERE_ALL_BITS, 1),
}


def _u32_scalar(x, what: str) -> int:
    """An integer in [0, 2**32) as an int; ValueError for a bool, a non-integer or a value outside."""
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise ValueError(f"{what} must be an integer, got {x!r}")
    if not 0 <= int(x) <= 0xFFFFFFFF:
        raise ValueError(f"{what} must lie in [0, 2**32), got {x!r}")
    return int(x)


def column_index(c) -> int:
    """A column number as an int; ValueError outside [0, COLUMNS_MAX)."""
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < COLUMNS_MAX:
        raise ValueError(f"column must be an integer in [0, {COLUMNS_MAX}), got {c!r}")
    return int(c)


COLLAPSE_ZERO = {"group": _native.COLLAPSE_ZERO_IS_GROUP, "single": _native.COLLAPSE_ZERO_SINGLE}


def collapse_zero_mode(zero) -> int:
    """``zero`` of a collapsed search -- "single": a row whose value is 0 is a group of its own; "group": 0 is a value
    like any other -- as svs_index_search_collapsed's zero_mode; ValueError for anything else."""
    if not isinstance(zero, str) or zero not in COLLAPSE_ZERO:
        raise ValueError(f"zero must be one of {sorted(COLLAPSE_ZERO)}, got {zero!r}")
    return COLLAPSE_ZERO[zero]


def _combined_batch(vectors, op, weights) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(vectors f32 (nq, m, D) contiguous, weights f32 (nq, m) or None) of a batch of combined queries; the shape, op
    and weight-shape errors of every combined entry are ValueErrors."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError(f"vectors must be (nq, m, D), got shape {v.shape}")
    nq, m, _ = v.shape
    if not 1 <= m <= COMBINE_MAX_VECTORS:
        raise ValueError(f"a combined query has 1 .. {COMBINE_MAX_VECTORS} vectors, got {m}")
    if op not in COMBINE_OPS:
        raise ValueError(f"op must be one of {sorted(COMBINE_OPS)}, got {op!r}")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.shape != (nq, m):
            raise ValueError(f"weights must be (nq, m) = {(nq, m)}, got shape {w.shape}")
    return v, w


def _combined_one(vectors, weights) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """One combined query, (m, D) and (m,) or None, as a batch of one."""
    v = np.asarray(vectors, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError(f"vectors must be (m, D), got shape {v.shape}")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32)
        if w.ndim != 1:
            raise ValueError(f"weights must be (m,), got shape {w.shape}")
        w = w[None, :]
    return v[None, :, :], w


def where_terms(where) -> list:
    """A ``where`` list -- terms ``(column, op, arg)``, all of which must hold -- checked and normalised to
    ``[(column, svs_where_op, negate, a, b, members)]``: ``members`` is the u32 vector of an in / not in term as given
    (the library sorts and deduplicates it) and None otherwise.  ``op`` is a key of WHERE_OPS; ``arg`` is an iterable of integers for in / not in,
    ``(lo, hi)`` for the range ops and an int mask for the bit ops.  ValueError for an unknown op, a bad column, a
    value that is negative, >= 2**32, a bool or no integer, more than WHERE_MAX_TERMS terms, or more than LABELS_MAX_SET
    distinct members over the call's sets."""
    terms = list(where)
    if len(terms) > WHERE_MAX_TERMS:
        raise ValueError(f"{len(terms)} terms; a predicate holds at most {WHERE_MAX_TERMS}")
    out, sets = [], []
    for term in terms:
        try:
            column, op, arg = term
        except (TypeError, ValueError):
            raise ValueError(f"a term is (column, op, arg), got {term!r}") from None
        column = column_index(column)
        if not isinstance(op, str) or op not in WHERE_OPS:
            raise ValueError(f"unknown op {op!r}; one of {sorted(WHERE_OPS)}")
        code, negate = WHERE_OPS[op]
        a = b = 0
        mem = None
        if code == _native.WHERE_IN:
            if isinstance(arg, (str, bytes)) or not hasattr(arg, "__iter__"):
                raise ValueError(f"{op!r} takes an iterable of integers, got {arg!r}")
            arg = arg if isinstance(arg, np.ndarray) else list(arg)
            if not isinstance(arg, np.ndarray) and any(isinstance(x, (bool, np.bool_)) for x in arg):
                raise ValueError("set members must be integers, got a bool")
            mem = labels_u32(arg)
            sets.append(mem)
        elif code == _native.WHERE_RANGE:
            try:
                lo, hi = arg
            except (TypeError, ValueError):
                raise ValueError(f"{op!r} takes (lo, hi), got {arg!r}") from None
            a, b = _u32_scalar(lo, "a range bound"), _u32_scalar(hi, "a range bound")
        else:
            a = _u32_scalar(arg, "a bit mask")
        out.append((column, code, negate, a, b, mem))
    # (distinct members are counted only when the members as given could exceed the limit)
    members = sum(len(m) for m in sets)
    if members > LABELS_MAX_SET:
        members = sum(len(np.unique(m)) for m in sets)
    if members > LABELS_MAX_SET:
        raise ValueError(f"{members} distinct set members over the in / not in terms; a call holds at most {LABELS_MAX_SET}")
    return out


def pack_where(where):
    """``where`` -> (the C array of svs_where_term_t or None, its length, what must stay alive during the call)."""
    terms = where_terms(where)
    if not terms:
        return None, 0, []
    arr = (_native.WhereTerm * len(terms))()
    keep = []
    for t, (column, code, negate, a, b, mem) in zip(arr, terms):
        t.column, t.op, t.negate, t.a, t.b = column, code, negate, a, b
        if mem is not None and len(mem):
            keep.append(mem)
            t.set, t.nset = mem.ctypes.data, len(mem)
        else:
            t.set, t.nset = None, 0
    return arr, len(terms), keep


def _query_1d(query_vec) -> np.ndarray:
    """The query of a single-query search as an f32 (D,) array."""
    q = np.asarray(query_vec, dtype=np.float32)
    if q.ndim != 1:
        raise ValueError(f"query must be 1-D, got shape {q.shape}")
    return q


def _means(sums: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Per-label sums (L, D) f64 and counts (L,) -> the means in f64; a label with count 0 gets zeros."""
    means = np.zeros(sums.shape, dtype=np.float64)
    has = counts > 0
    means[has] = sums[has] / counts[has, None].astype(np.float64)
    return means


def _centroids(sums: np.ndarray, counts: np.ndarray, previous: np.ndarray, spherical: bool) -> np.ndarray:
    """The update step of ``DeviceIndex.kmeans``: the means (``spherical``: normalised to unit length) in f64, cast
    to f32; a label with count 0, or with a zero-norm sum, keeps its row of ``previous``."""
    cent = _means(sums, counts)
    norm = np.sqrt((cent * cent).sum(axis=1))
    keep = (counts == 0) | ~(norm > 0.0)
    if spherical:
        cent[~keep] = cent[~keep] / norm[~keep, None]
    out = cent.astype(np.float32)
    out[keep] = previous[keep]
    return out


class DeviceIndex:
    """One shard of a corpus, resident in the HBM of one MI355X.

    ``matrix`` is the array ``_Querier.build_embeddings_matrix`` returns
    (reference src/svs/kb.py:600): float32, shape (N, D), C-contiguous.  It is
    copied once (pinned staging -> HBM); the caller keeps ownership.
    """

    def __init__(self, matrix: Optional[np.ndarray], device: int = 0, row_offset: int = 0,
                 dtype: str = "f32", *, _handle: Optional[int] = None):
        self._lib = _native.load()
        self._quick = _native.quick()   # info / retain / release of a per-call reference: under the GIL (see _native.QUICK)
        self._lock = threading.Lock()
        self._h: Optional[int] = None
        if _handle is not None:
            self._h = _handle
        else:
            assert matrix is not None
            m = np.asarray(matrix)
            if m.ndim != 2:
                raise ValueError(f"embeddings matrix must be 2-D, got shape {m.shape}")
            if m.dtype != np.float32 or not m.flags["C_CONTIGUOUS"]:
                m = np.ascontiguousarray(m, dtype=np.float32)
            out = C.c_void_p()
            _native.check(self._lib.svs_index_create(
                m.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], _DTYPES[dtype],
                int(device), int(row_offset), C.byref(out)))
            self._h = out.value
        self._refresh()

    def _refresh(self) -> None:
        info = _native.IndexInfo()
        _native.check(self._lib.svs_index_info(self._handle(), C.byref(info)))
        self.n, self.d, self.ld = int(info.n), int(info.d), int(info.ld)
        self.device, self.row_offset = int(info.device), int(info.row_offset)
        self.hbm_bytes = int(info.hbm_bytes)
        self.n_masked = int(info.n_masked)
        self.dtype = {v: k for k, v in _DTYPES.items()}[int(info.dtype)]

    @classmethod
    def from_device_pointer(cls, ptr: int, n: int, d: int, src_ld: Optional[int] = None,
                            device: int = 0, row_offset: int = 0, dtype: str = "f32") -> "DeviceIndex":
        """Corpus rows already in device memory (f32): copies them into the
        index's own HBM layout.  ``ptr`` is a raw device address (e.g.
        ``tensor.data_ptr()``)."""
        lib = _native.load()
        out = C.c_void_p()
        _native.check(lib.svs_index_create_from_device(
            C.c_void_p(ptr), int(n), int(d), int(src_ld if src_ld is not None else d),
            _DTYPES[dtype], int(device), int(row_offset), C.byref(out)))
        return cls(None, _handle=out.value)

    # -- lifetime ---------------------------------------------------------
    @property
    def shape(self) -> Tuple[int, int]:
        return (self.n, self.d)

    def __len__(self) -> int:
        return self.n

    def _handle(self) -> int:
        h = self._h
        if h is None:
            raise RuntimeError("DeviceIndex has been released")
        return h

    def release(self) -> None:
        """Drops this object's reference; in-flight searches on other threads
        keep the HBM alive until they finish (ref-counted in the library)."""
        with self._lock:
            h, self._h = self._h, None
        if h is not None:
            self._lib.svs_index_release(h)

    close = release

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def _live_rows(self, h: Optional[int] = None) -> int:
        """Rows a search can return right now (the handle may have been appended to or
        masked through another owner since this object last looked).  ``h``: a pinned handle to ask."""
        info = _native.IndexInfo()
        _native.check(self._quick.svs_index_info(self._handle() if h is None else h, C.byref(info)))
        return max(int(info.n) - int(info.n_masked), 0)

    @staticmethod
    def _queries_2d(queries) -> np.ndarray:
        """The queries of a batched search as a C-contiguous f32 (nq, D) array."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError(f"queries must be 2-D, got shape {q.shape}")
        return q

    @staticmethod
    def _trimmed(scores: np.ndarray, rows: np.ndarray, count: int) -> Tuple[np.ndarray, np.ndarray]:
        """Both (nq, k) result arrays cut to the ``count`` entries per query the library wrote."""
        return (scores, rows) if count == scores.shape[1] else (scores[:, :count], rows[:, :count])

    def _pinned_handle(self) -> int:
        """retain() under the lock so a concurrent release() cannot free the
        handle between reading it and entering the library."""
        with self._lock:
            h = self._handle()
            self._quick.svs_index_retain(h)
            return h

    def _unpin(self, h: int) -> None:
        """Drops the reference _pinned_handle() took (normally not the last one: the owner holds its own)."""
        self._quick.svs_index_release(h)

    # -- incremental update ---------------------------------
    def append(self, matrix: np.ndarray) -> None:
        """New rows behind the existing ones (what a rebuilt matrix would hold after
        ``bulk_add_docs``), without re-uploading the corpus."""
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        if m.ndim != 2 or (m.shape[0] and m.shape[1] != self.d):
            raise ValueError(f"cannot append shape {m.shape} to an index of dimension {self.d}")
        _native.check(self._lib.svs_index_append(self._handle(), m.ctypes.data_as(C.c_void_p), m.shape[0]))
        self._refresh()

    @classmethod
    def empty(cls, d: int, device: int = 0, row_offset: int = 0, dtype: str = "f32",
              reserve: int = 0) -> "DeviceIndex":
        """An index of dimension ``d`` with no rows yet (optionally with room for ``reserve`` rows),
        to be filled with ``append`` / ``append_device`` block by block -- the way a cold start
        streams BLOBs out of SQLite without ever holding the whole matrix on the host."""
        lib = _native.load()
        out = C.c_void_p()
        _native.check(lib.svs_index_create(None, 0, int(d), _DTYPES[dtype], int(device), int(row_offset), C.byref(out)))
        idx = cls(None, _handle=out.value)
        if reserve > 0:
            idx.reserve(reserve)
        return idx

    def reserve(self, rows: int) -> None:
        _native.check(self._lib.svs_index_reserve(self._handle(), int(rows)))
        self._refresh()

    def append_device(self, ptr: int, n: int, src_ld: Optional[int] = None) -> None:
        """``append`` for f32 rows already in this device's memory (raw device address)."""
        _native.check(self._lib.svs_index_append_from_device(
            self._handle(), C.c_void_p(ptr), int(n), int(src_ld if src_ld is not None else self.d)))
        self._refresh()

    # -- cold start: BLOBs decoded straight into the library's pinned staging blocks --------------
    def staging_acquire(self) -> np.ndarray:
        """A (rows_cap, d) float32 array over pinned memory owned by the library: fill its first rows,
        then ``staging_commit(n)``.  Two blocks alternate; the DMA of one overlaps the filling of the other."""
        ptr, cap = C.c_void_p(), C.c_int64(0)
        _native.check(self._lib.svs_index_staging_acquire(self._handle(), C.byref(ptr), C.byref(cap)))
        buf = (C.c_float * (cap.value * self.d)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(cap.value, self.d)

    def staging_commit(self, n_rows: int) -> None:
        _native.check(self._lib.svs_index_staging_commit(self._handle(), int(n_rows)))
        self._refresh()      # the library publishes the new row count at commit: keep the wrapper's in step

    def staging_finish(self) -> None:
        _native.check(self._lib.svs_index_staging_finish(self._handle()))
        self._refresh()

    def mask_rows(self, rows) -> None:
        """Tombstone rows (global indices): they are never returned again; the other
        rows keep their indices."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        _native.check(self._lib.svs_index_mask_rows(self._handle(), r.ctypes.data_as(C.c_void_p), r.shape[0]))
        self._refresh()

    def compact(self, bounce_rows: int = 0, stats: Optional[list] = None) -> np.ndarray:
        """Physically removes the tombstoned rows, in place in HBM (svs_index_compact): live row r becomes
        r - (dead rows below r), ``n`` shrinks, ``n_masked`` becomes 0.  Returns the old GLOBAL row of every new row
        (i64, one per row left).  Row indices obtained before the call are stale after it.  ``bounce_rows`` / ``stats``
        (a list that receives DIRECT steps, BOUNCE steps, rows moved, bytes moved) go through svs_internal_compact:
        tests and tools."""
        h = self._pinned_handle()
        try:
            live = self._live_rows(h)
            for _ in range(8):
                # (rows appended through another owner since the map was sized: the call reports the count to retry with)
                out = np.empty(live, dtype=np.int64)
                now = C.c_int64(0)
                if bounce_rows or stats is not None:
                    st = (C.c_int64 * 4)()
                    rc = self._lib.svs_internal_compact(h, int(bounce_rows), out.ctypes.data_as(C.c_void_p), live, C.byref(now), st)
                    if stats is not None:
                        stats[:] = [int(v) for v in st]
                else:
                    rc = self._lib.svs_index_compact(h, out.ctypes.data_as(C.c_void_p), live, C.byref(now))
                if rc == _native.SVS_OK or now.value <= live:
                    break
                live = now.value
            _native.check(rc)
        finally:
            self._unpin(h)
        self._refresh()
        return out[:now.value]

    def share(self) -> "DeviceIndex":
        """A second owner of the same HBM copy (its own reference): what an
        in-flight AsyncKB search holds so that ``invalidate()`` on another task
        cannot pull the corpus from under it (reference semantics: the closure
        keeps the numpy arrays alive, src/svs/kb.py:1180-1190)."""
        return DeviceIndex(None, _handle=self._pinned_handle())

    # -- search -----------------------------------------------------------
    def search_batch(self, queries: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """Top-n for each row of ``queries`` (nq, D).  Returns
        (scores f32 (nq, count), rows i64 (nq, count)), count = min(max(n,0), N),
        each row ordered (score desc, row desc)."""
        assert isinstance(n, int)  # reference src/svs/util.py:197
        q = self._queries_2d(queries)
        nq, d = q.shape
        h = self._pinned_handle()
        try:
            # clamp before allocating and before the int32 argument (reference src/svs/util.py:198-199
            # clamps top_k to len(scores) first): k = 2**32 must mean "rank everything", not 0.  (The row count is
            # read through the pinned handle: the index may have been appended to or masked through another owner.)
            k = min(max(n, 0), self._live_rows(h))
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            count = C.c_int32(0)
            # (the one call of a search that releases the GIL)
            _native.check(self._lib.svs_index_search(h, q.ctypes.data, nq, d, k, scores.ctypes.data, rows.ctypes.data,
                                                     C.byref(count)))
        finally:
            self._unpin(h)
        return self._trimmed(scores, rows, count.value)

    def search(self, query_vec: np.ndarray, n: int) -> List[Tuple[float, int]]:
        """``get_top_k(np.dot(M, query_vec), n)``: list of (score, row index),
        python float / python int, as the reference returns them."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r = self.search_batch(q[None, :], n)
        # (tolist(): python floats -- the exact widening float(np.float32) does, src/svs/util.py:203 -- and ints in C)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist()))

    def search_batch_within(self, queries: np.ndarray, n: int, rows) -> Tuple[np.ndarray, np.ndarray]:
        """``search_batch`` over the listed rows only (GLOBAL indices, any order, duplicates allowed;
        masked rows drop out): (scores f32 (nq, count), rows i64 (nq, count)), count = min(max(n, 0),
        live listed rows), each row ordered (score desc, row desc) -- ``get_top_k(np.dot(M[S], q), n)``
        with positions mapped back to rows S (svs_index_search_rows)."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        nq, d = q.shape
        k = min(max(n, 0), len(r), 2 ** 31 - 1)   # (count <= listed rows: clamp before allocating)
        scores = np.empty((nq, k), dtype=np.float32)
        out_rows = np.empty((nq, k), dtype=np.int64)
        count = C.c_int32(0)
        h = self._pinned_handle()
        try:
            _native.check(self._lib.svs_index_search_rows(h, q.ctypes.data, nq, d, k, r.ctypes.data, len(r),
                                                          scores.ctypes.data, out_rows.ctypes.data, C.byref(count)))
        finally:
            self._unpin(h)
        return self._trimmed(scores, out_rows, count.value)

    def search_within(self, query_vec: np.ndarray, n: int, rows) -> List[Tuple[float, int]]:
        """``search`` restricted to the listed rows (see ``search_batch_within``): [(score, row)]."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r = self.search_batch_within(q[None, :], n, rows)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist()))

    def search_segments(self, queries: np.ndarray, n: int, row_lists, seg_query=None) -> List[Tuple[np.ndarray, np.ndarray]]:
        """``search_within`` for MANY row lists in one call (svs_index_search_segments): segment s is
        ``row_lists[s]`` (GLOBAL rows, any order, duplicates allowed, masked rows drop out) searched with query
        ``seg_query[s]`` of ``queries`` (nq, D) -- ``seg_query=None``: with query s, one list per query.  Returns one
        ``(scores f32 (count_s,), rows i64 (count_s,))`` per segment, count_s = min(max(n, 0), live listed rows of s),
        ordered (score desc, row desc): the rows and score bits ``search_within(queries[seg_query[s]], n,
        row_lists[s])`` gives.  Nothing is merged across segments."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        lists = [np.asarray(r, dtype=np.int64).reshape(-1) for r in row_lists]
        nseg = len(lists)
        nq, d = q.shape
        begin = np.zeros(nseg + 1, dtype=np.int64)
        if nseg:
            np.cumsum([len(r) for r in lists], out=begin[1:])
        rows = np.concatenate(lists) if nseg else np.zeros(0, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        sq = None
        if seg_query is not None:
            sq = np.ascontiguousarray(seg_query, dtype=np.int32).reshape(-1)
            if len(sq) != nseg:
                raise ValueError(f"seg_query has {len(sq)} entries for {nseg} row lists")
        longest = max((len(r) for r in lists), default=0)
        k = min(max(n, 0), longest, 2 ** 31 - 1)   # (count_s <= listed rows of s: clamp before allocating)
        scores = np.empty((nseg, k), dtype=np.float32)
        out_rows = np.empty((nseg, k), dtype=np.int64)
        counts = np.zeros(nseg, dtype=np.int32)
        h = self._pinned_handle()
        try:
            _native.check(self._lib.svs_index_search_segments(h, q.ctypes.data, nq, d, k, rows.ctypes.data, begin.ctypes.data,
                                                              None if sq is None else sq.ctypes.data, nseg, scores.ctypes.data,
                                                              out_rows.ctypes.data, counts.ctypes.data))
        finally:
            self._unpin(h)
        return [(scores[s, :c], out_rows[s, :c]) for s, c in enumerate(counts.tolist())]

    def search_batch_above(self, queries: np.ndarray, min_scores, limit: int) -> List[Tuple[np.ndarray, np.ndarray, int]]:
        """Threshold search (svs_index_search_above): for each row of ``queries`` (nq, D) every live row whose score
        is at or above ``min_scores[q]`` -- compared in the key space of the top-k order: -0.0 == +0.0, a NaN score
        qualifies for every cut-off and sorts first -- best first, at most ``limit`` of them.  Returns one
        ``(scores f32 (count,), rows i64 (count,), total)`` per query: count = min(max(limit, 0), total), total = the
        number of qualifying rows, exact however large.  ``limit=0`` only counts.  A NaN cut-off is a ValueError."""
        assert isinstance(limit, int)
        q = self._queries_2d(queries)
        nq, d = q.shape
        cut = np.ascontiguousarray(min_scores, dtype=np.float32).reshape(-1)
        if len(cut) != nq:
            raise ValueError(f"min_scores has {len(cut)} entries for {nq} queries")
        if np.isnan(cut).any():
            raise ValueError(f"the cut-off of query {int(np.argmax(np.isnan(cut)))} is NaN")
        h = self._pinned_handle()
        try:
            # (clamped before allocating and before the int32 argument, as in search_batch)
            k = min(max(limit, 0), self._live_rows(h))
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            counts = np.zeros(nq, dtype=np.int32)
            totals = np.zeros(nq, dtype=np.int64)
            # (the one call that releases the GIL; a count-only call passes no result buffers)
            _native.check(self._lib.svs_index_search_above(h, q.ctypes.data, nq, d, cut.ctypes.data, k,
                                                           scores.ctypes.data if k else None, rows.ctypes.data if k else None,
                                                           counts.ctypes.data, totals.ctypes.data))
        finally:
            self._unpin(h)
        return [(scores[i, :c], rows[i, :c], t) for i, (c, t) in enumerate(zip(counts.tolist(), totals.tolist()))]

    def search_above(self, query_vec: np.ndarray, min_score: float, limit: int) -> Tuple[List[Tuple[float, int]], int]:
        """Every live row scoring at or above ``min_score``, best first, at most ``limit``: ([(score, row)], total),
        total = how many rows qualify (``limit=0``: only that).  See ``search_batch_above``."""
        assert isinstance(limit, int)
        q = _query_1d(query_vec)
        s, r, total = self.search_batch_above(q[None, :], [min_score], limit)[0]
        return list(zip(s.astype(np.float64).tolist(), r.tolist())), total

    # -- labels: one u32 per row in HBM, and the search that names them (svs_index_search_labeled) ----------------
    def set_labels(self, labels, row0: Optional[int] = None) -> None:
        """``labels`` (integers in [0, 2**32)) become the labels of the GLOBAL rows ``row0 .. row0 + len(labels)``
        (``row0=None``: from the index's first row).  The column lives in HBM only; a row never labelled carries 0, and
        rows appended later get 0 (svs_index_set_labels)."""
        lab = labels_u32(labels)
        r0 = self.row_offset if row0 is None else int(row0)
        _native.check(self._lib.svs_index_set_labels(self._handle(), r0, len(lab), lab.ctypes.data))
        self._refresh()      # (the first call allocates the column: hbm_bytes)

    def labels(self, row0: Optional[int] = None, nrows: Optional[int] = None) -> np.ndarray:
        """The labels of the GLOBAL rows ``row0 .. row0 + nrows`` as the DEVICE holds them, u32 (``row0=None``: from the
        first row; ``nrows=None``: to the last).  Zeros when no label was ever set (svs_index_get_labels)."""
        h = self._pinned_handle()
        try:
            info = _native.IndexInfo()
            _native.check(self._quick.svs_index_info(h, C.byref(info)))
            r0 = int(info.row_offset) if row0 is None else int(row0)
            cnt = int(info.row_offset) + int(info.n) - r0 if nrows is None else int(nrows)
            out = np.empty(max(cnt, 0), dtype=np.uint32)
            _native.check(self._lib.svs_index_get_labels(h, r0, cnt, out.ctypes.data))
        finally:
            self._unpin(h)
        return out

    def _search_batch_filtered(self, native_search, queries, n: int, filter_arg, filter_len: int) -> Tuple[np.ndarray, np.ndarray, int]:
        """``search_batch_labeled`` / ``search_batch_where``: ``native_search`` is the bound entry, ``filter_arg`` and
        ``filter_len`` its two filter arguments (the caller keeps what they point to alive)."""
        q = self._queries_2d(queries)
        nq, d = q.shape
        h = self._pinned_handle()
        try:
            # (clamped before allocating and before the int32 argument, as in search_batch)
            k = min(max(n, 0), self._live_rows(h))
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            count, matched = C.c_int32(0), C.c_int64(0)
            # (the one call that releases the GIL)
            _native.check(native_search(h, q.ctypes.data, nq, d, k, filter_arg, filter_len,
                                        scores.ctypes.data, rows.ctypes.data, C.byref(count), C.byref(matched)))
        finally:
            self._unpin(h)
        return self._trimmed(scores, rows, count.value) + (matched.value,)

    def search_batch_labeled(self, queries: np.ndarray, n: int, labels) -> Tuple[np.ndarray, np.ndarray, int]:
        """``search_batch`` over the live rows whose label is in ``labels`` (any order, repeats allowed, at most
        LABELS_MAX_SET distinct ones; none: the empty set): (scores f32 (nq, count), rows i64 (nq, count), matched),
        matched = how many rows carry such a label, count = min(max(n, 0), matched), each row ordered (score desc,
        row desc) -- the rows and score bits ``search_batch_within`` gives for exactly those rows, with the filter run on
        the device (svs_index_search_labeled).  ``n=0`` only counts."""
        assert isinstance(n, int)
        lab = labels_u32(labels)
        return self._search_batch_filtered(self._lib.svs_index_search_labeled, queries, n, lab.ctypes.data, len(lab))

    def search_labeled(self, query_vec: np.ndarray, n: int, labels) -> Tuple[List[Tuple[float, int]], int]:
        """``search`` restricted to the rows whose label is in ``labels`` (see ``search_batch_labeled``):
        ([(score, row)], matched)."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, matched = self.search_batch_labeled(q[None, :], n, labels)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist())), matched

    # -- columns and predicate search (svs_index_set_column, svs_index_search_where) -------------------------------
    def set_column(self, c: int, values, row0: Optional[int] = None) -> None:
        """``values`` (integers in [0, 2**32)) become column ``c``'s values of the GLOBAL rows ``row0 .. row0 +
        len(values)`` (``row0=None``: from the index's first row).  Column 0 is the label column (``set_labels``);
        every column lives in HBM only, a row never set reads 0 and rows appended later get 0 (svs_index_set_column)."""
        c = column_index(c)
        val = labels_u32(values)
        r0 = self.row_offset if row0 is None else int(row0)
        _native.check(self._lib.svs_index_set_column(self._handle(), c, r0, len(val), val.ctypes.data))
        self._refresh()      # (the first call allocates the column: hbm_bytes)

    def column(self, c: int, row0: Optional[int] = None, nrows: Optional[int] = None) -> np.ndarray:
        """Column ``c`` of the GLOBAL rows ``row0 .. row0 + nrows`` as the DEVICE holds it, u32 (``row0=None``: from the
        first row; ``nrows=None``: to the last).  Zeros for a column never set (svs_index_get_column)."""
        c = column_index(c)
        h = self._pinned_handle()
        try:
            info = _native.IndexInfo()
            _native.check(self._quick.svs_index_info(h, C.byref(info)))
            r0 = int(info.row_offset) if row0 is None else int(row0)
            cnt = int(info.row_offset) + int(info.n) - r0 if nrows is None else int(nrows)
            out = np.empty(max(cnt, 0), dtype=np.uint32)
            _native.check(self._lib.svs_index_get_column(h, c, r0, cnt, out.ctypes.data))
        finally:
            self._unpin(h)
        return out

    def search_batch_where(self, queries: np.ndarray, n: int, where) -> Tuple[np.ndarray, np.ndarray, int]:
        """``search_batch`` over the live rows on which every term of ``where`` holds (``where_terms``; no term: every
        live row): (scores f32 (nq, count), rows i64 (nq, count), matched), matched = how many rows satisfy the
        predicate, count = min(max(n, 0), matched), each row ordered (score desc, row desc) -- the rows and score bits
        ``search_batch_within`` gives for exactly those rows, with the filter run on the device
        (svs_index_search_where).  ``n=0`` only counts."""
        assert isinstance(n, int)
        terms, nterms, keep = pack_where(where)
        out = self._search_batch_filtered(self._lib.svs_index_search_where, queries, n, terms, nterms)
        del keep
        return out

    def search_where(self, query_vec: np.ndarray, n: int, where) -> Tuple[List[Tuple[float, int]], int]:
        """``search`` restricted to the rows on which every term of ``where`` holds (see ``search_batch_where``):
        ([(score, row)], matched)."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, matched = self.search_batch_where(q[None, :], n, where)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist())), matched

    def count_where(self, where) -> int:
        """How many live rows satisfy ``where``: the counting launch alone (svs_index_search_where with k = 0)."""
        terms, nterms, keep = pack_where(where)
        h = self._pinned_handle()
        try:
            matched = C.c_int64(0)
            _native.check(self._lib.svs_index_search_where(h, None, 0, self.d, 0, terms, nterms, None, None, None, C.byref(matched)))
        finally:
            self._unpin(h)
        del keep
        return int(matched.value)

    def search_batch_by_label(self, queries: np.ndarray, labels, min_scores=None,
                              n: Optional[int] = None) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]]:
        """Per-label breakdown (svs_index_search_by_label): for each row of ``queries`` (nq, D) and every label of
        ``labels`` (any order, repeats allowed, at most LABELS_MAX_SET distinct ones) the number of live rows of that
        label scoring at or above ``min_scores[q]`` (None: every live row; compared in key space as in
        ``search_batch_above``) and the best of them.  Returns one ``(labels u32, scores f32, rows i64, totals i64,
        groups)`` per query: the labels that have a qualifying row ordered by their best row (score desc, row desc), at
        most ``n`` of them (None: every label of the set; 0: only ``groups``); groups = how many labels have one.
        A NaN cut-off is a ValueError."""
        assert n is None or isinstance(n, int)
        q = self._queries_2d(queries)
        nq, d = q.shape
        lab = labels_u32(labels)
        cut = None
        if min_scores is not None:
            cut = np.ascontiguousarray(min_scores, dtype=np.float32).reshape(-1)
            if len(cut) != nq:
                raise ValueError(f"min_scores has {len(cut)} entries for {nq} queries")
            if np.isnan(cut).any():
                raise ValueError(f"the cut-off of query {int(np.argmax(np.isnan(cut)))} is NaN")
        # (clamped before allocating and before the int32 argument: a query has at most one entry per label given)
        k = len(lab) if n is None else min(max(n, 0), len(lab))
        out_l = np.empty((nq, k), dtype=np.uint32)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        out_t = np.empty((nq, k), dtype=np.int64)
        counts = np.zeros(nq, dtype=np.int32)
        groups = np.zeros(nq, dtype=np.int32)
        h = self._pinned_handle()
        try:
            # (the one call that releases the GIL; a count-only call passes no result buffers)
            _native.check(self._lib.svs_index_search_by_label(h, q.ctypes.data, nq, d, lab.ctypes.data, len(lab),
                                                              None if cut is None else cut.ctypes.data, k,
                                                              out_l.ctypes.data if k else None, out_s.ctypes.data if k else None,
                                                              out_r.ctypes.data if k else None, out_t.ctypes.data if k else None,
                                                              counts.ctypes.data, groups.ctypes.data))
        finally:
            self._unpin(h)
        return [(out_l[i, :c], out_s[i, :c], out_r[i, :c], out_t[i, :c], g) for i, (c, g) in enumerate(zip(counts.tolist(), groups.tolist()))]

    def search_by_label(self, query_vec: np.ndarray, labels, min_score: Optional[float] = None,
                        n: Optional[int] = None) -> List[Tuple[int, float, int, int]]:
        """The breakdown of one query over ``labels``: [(label, score of its best row, that row, rows of the label at or
        above ``min_score``)], best label first; labels without such a row are absent.  See ``search_batch_by_label``."""
        q = _query_1d(query_vec)
        l, s, r, t, _ = self.search_batch_by_label(q[None, :], labels, None if min_score is None else [min_score], n)[0]
        return list(zip(l.tolist(), s.astype(np.float64).tolist(), r.tolist(), t.tolist()))

    def search_batch_collapsed(self, queries: np.ndarray, n: int, column: int,
                               zero: str = "single") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Collapsed search (svs_index_search_collapsed): for each row of ``queries`` (nq, D) the ``n`` best live rows
        with at most ONE row per value of column ``column`` -- every value is represented by its best row (score
        desc, row desc in key space).  ``zero="single"``: a row whose value is 0 ("no parent") stands for itself;
        ``zero="group"``: 0 is a value like any other.  Returns ``(scores f32 (nq, k), rows i64 (nq, k), values u32
        (nq, k), counts i32 (nq,), groups i64 (nq,))`` with k = min(max(n, 0), live rows): query i has counts[i] =
        min(k, groups[i]) valid entries, groups[i] = how many rows are the best of their group; the entries past
        counts[i] are unspecified.  ``n=0`` only counts the groups."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        nq, d = q.shape
        c = column_index(column)
        mode = collapse_zero_mode(zero)
        h = self._pinned_handle()
        try:
            # (clamped before allocating and before the int32 argument, as in search_batch)
            k = min(max(n, 0), self._live_rows(h))
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            values = np.empty((nq, k), dtype=np.uint32)
            counts = np.zeros(nq, dtype=np.int32)
            groups = np.zeros(nq, dtype=np.int64)
            # (the one call that releases the GIL; a count-only call passes no result buffers)
            _native.check(self._lib.svs_index_search_collapsed(h, q.ctypes.data, nq, d, k, c, mode,
                                                               scores.ctypes.data if k else None, rows.ctypes.data if k else None,
                                                               values.ctypes.data if k else None, counts.ctypes.data, groups.ctypes.data))
        finally:
            self._unpin(h)
        return scores, rows, values, counts, groups

    def search_collapsed(self, query_vec: np.ndarray, n: int, column: int, zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int]:
        """The ``n`` best rows of one query with at most one row per value of column ``column``: ([(score, row,
        value)], groups), best first.  See ``search_batch_collapsed``."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, v, counts, groups = self.search_batch_collapsed(q[None, :], n, column, zero)
        c = int(counts[0])
        return list(zip(s[0, :c].astype(np.float64).tolist(), r[0, :c].tolist(), v[0, :c].tolist())), int(groups[0])

    def _search_batch_collapsed_scoped(self, native_search, q: np.ndarray, n: int, scope_arg, scope_len: int, scope_rows: Optional[int],
                                       c: int, mode: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """``search_batch_collapsed_where`` / ``search_batch_collapsed_within`` once their arguments are checked:
        ``native_search`` is the bound entry, ``scope_arg`` and ``scope_len`` its two scope arguments (the caller keeps
        what they point to alive), ``scope_rows`` a bound on the rows in scope the caller knows (None: none)."""
        nq, d = q.shape
        h = self._pinned_handle()
        try:
            # (clamped before allocating and before the int32 argument, as in search_batch)
            k = min(max(n, 0), self._live_rows(h), 2 ** 31 - 1 if scope_rows is None else scope_rows)
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            values = np.empty((nq, k), dtype=np.uint32)
            counts = np.zeros(nq, dtype=np.int32)
            groups = np.zeros(nq, dtype=np.int64)
            matched = C.c_int64(0)
            # (the one call that releases the GIL; a count-only call passes no result buffers)
            _native.check(native_search(h, q.ctypes.data, nq, d, k, scope_arg, scope_len, c, mode,
                                        scores.ctypes.data if k else None, rows.ctypes.data if k else None,
                                        values.ctypes.data if k else None, counts.ctypes.data, groups.ctypes.data, C.byref(matched)))
        finally:
            self._unpin(h)
        return scores, rows, values, counts, groups, int(matched.value)

    def search_batch_collapsed_where(self, queries: np.ndarray, n: int, where, column: int,
                                     zero: str = "single") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """``search_batch_collapsed`` inside the scope of a predicate (svs_index_search_collapsed_where): only the live
        rows on which every term of ``where`` holds (``where_terms``; no term: every live row) are scored and grouped,
        so a value is represented by its best row IN SCOPE and a value with no row in scope is absent.  Returns
        ``(scores, rows, values, counts, groups, matched)``: ``search_batch_collapsed``'s five, k = min(max(n, 0), live
        rows), and matched = how many rows satisfy the predicate.  The scores are the bits ``search_batch_where``
        reports for those rows.  ``n=0`` only counts."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        c = column_index(column)
        mode = collapse_zero_mode(zero)
        terms, nterms, keep = pack_where(where)
        out = self._search_batch_collapsed_scoped(self._lib.svs_index_search_collapsed_where, q, n, terms, nterms, None, c, mode)
        del keep
        return out

    def search_collapsed_where(self, query_vec: np.ndarray, n: int, where, column: int,
                               zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int, int]:
        """The ``n`` best rows of one query among the rows ``where`` admits, at most one per value of column
        ``column``: ([(score, row, value)], groups, matched), best first.  See ``search_batch_collapsed_where``."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, v, counts, groups, matched = self.search_batch_collapsed_where(q[None, :], n, where, column, zero)
        c = int(counts[0])
        return list(zip(s[0, :c].astype(np.float64).tolist(), r[0, :c].tolist(), v[0, :c].tolist())), int(groups[0]), matched

    def search_batch_collapsed_within(self, queries: np.ndarray, n: int, rows, column: int,
                                      zero: str = "single") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """``search_batch_collapsed`` inside the scope of a row list (svs_index_search_collapsed_rows): ``rows`` are
        GLOBAL indices, any order, duplicates allowed; masked rows drop out.  Returns what
        ``search_batch_collapsed_where`` returns, k = min(max(n, 0), listed rows), matched = the distinct live listed
        rows; the scores are the bits ``search_batch_within`` reports for them."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        c = column_index(column)
        mode = collapse_zero_mode(zero)
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        return self._search_batch_collapsed_scoped(self._lib.svs_index_search_collapsed_rows, q, n, r.ctypes.data, len(r), len(r), c, mode)

    def search_collapsed_within(self, query_vec: np.ndarray, n: int, rows, column: int,
                                zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int, int]:
        """The ``n`` best rows of one query among the listed rows, at most one per value of column ``column``:
        ([(score, row, value)], groups, matched), best first.  See ``search_batch_collapsed_within``."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, v, counts, groups, matched = self.search_batch_collapsed_within(q[None, :], n, rows, column, zero)
        c = int(counts[0])
        return list(zip(s[0, :c].astype(np.float64).tolist(), r[0, :c].tolist(), v[0, :c].tolist())), int(groups[0]), matched

    def assign(self, vectors, labels=None, row0: Optional[int] = None, nrows: Optional[int] = None,
               scores: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
        """Nearest-vector assignment (svs_index_assign): for each of the GLOBAL rows ``row0 .. row0 + nrows`` (default:
        the whole index), live or tombstoned, the position of the row of ``vectors`` (c, D; at most ASSIGN_MAX_VECTORS)
        it scores best against -- both as stored, an exact tie to the lower position.  Returns ``(best i32 (nrows,),
        scores f32 (nrows,) or None with scores=False, counts i64 (c,))``; counts[j] = the LIVE rows of the range
        assigned to j.  ``labels`` (c integers in [0, 2**32)): label[row] = labels[best[row]] is also written into the
        label column for every row of the range; None: the column is not touched.  ValueError for shape and argument
        errors, NotImplementedError for more than ASSIGN_MAX_VECTORS vectors."""
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2:
            raise ValueError(f"vectors must be 2-D (c, D), got shape {v.shape}")
        c, d = v.shape
        lab = None
        if labels is not None:
            lab = labels_u32(labels)
            if len(lab) != c:
                raise ValueError(f"{len(lab)} labels for {c} vectors")
        h = self._pinned_handle()
        try:
            info = _native.IndexInfo()
            _native.check(self._quick.svs_index_info(h, C.byref(info)))
            r0 = int(info.row_offset) if row0 is None else int(row0)
            cnt = int(info.row_offset) + int(info.n) - r0 if nrows is None else int(nrows)
            best = np.empty(max(cnt, 0), dtype=np.int32)
            sc = np.empty(max(cnt, 0), dtype=np.float32) if scores else None
            counts = np.zeros(max(c, 0), dtype=np.int64)
            # (the one call that releases the GIL)
            _native.check(self._lib.svs_index_assign(h, v.ctypes.data if v.size else None, c, d, r0, cnt,
                                                     None if lab is None else lab.ctypes.data, best.ctypes.data,
                                                     None if sc is None else sc.ctypes.data, counts.ctypes.data))
        finally:
            self._unpin(h)
        if lab is not None:
            self._refresh()      # (the first labelled call allocates the column: hbm_bytes)
        return best, sc, counts

    def label_sums(self, labels, row_labels=None, row0: Optional[int] = None, nrows: Optional[int] = None,
                   sums: bool = True) -> Tuple[Optional[np.ndarray], np.ndarray]:
        """Per-label row sums (svs_index_label_sums): for every entry of ``labels`` (L integers in [0, 2**32), any order,
        repeats allowed, at most LABELS_MAX_SET distinct ones) the f64 sum of the stored values of the LIVE rows among
        the GLOBAL rows ``row0 .. row0 + nrows`` (default: the whole index) that carry the label, and their number.  A
        row's label is ``row_labels[row - row0]`` when ``row_labels`` (one integer per row of the range, e.g. the
        ``best`` of ``assign``) is given, else the label column's.  Returns ``(sums f64 (L, D) or None with sums=False,
        counts i64 (L,))``; ``sums=False`` runs the histogram only.  The sum is a fixed tree of f64 additions (chunks of
        256 rows in ascending row order): bit-reproducible, and exact whenever its partial sums are representable.
        ValueError for argument errors, NotImplementedError for too many labels or rows of more than 16 KiB."""
        lab = labels_u32(labels)
        rl = None if row_labels is None else labels_u32(row_labels)
        h = self._pinned_handle()
        try:
            info = _native.IndexInfo()
            _native.check(self._quick.svs_index_info(h, C.byref(info)))
            r0 = int(info.row_offset) if row0 is None else int(row0)
            cnt = int(info.row_offset) + int(info.n) - r0 if nrows is None else int(nrows)
            if rl is not None and len(rl) != cnt:
                raise ValueError(f"{len(rl)} row labels for {cnt} rows")
            out = np.zeros((len(lab), int(info.d)), dtype=np.float64) if sums else None
            counts = np.zeros(len(lab), dtype=np.int64)
            # (the one call that releases the GIL)
            _native.check(self._lib.svs_index_label_sums(h, lab.ctypes.data if len(lab) else None, len(lab), r0, cnt,
                                                         None if rl is None or not len(rl) else rl.ctypes.data,
                                                         None if out is None else out.ctypes.data, counts.ctypes.data))
        finally:
            self._unpin(h)
        return out, counts

    def label_means(self, labels, row_labels=None, row0: Optional[int] = None,
                    nrows: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """``label_sums`` divided by the counts in f64, then cast: ``(means f32 (L, D), counts i64 (L,))``; a label
        without a live row gets an all-zero mean."""
        s, counts = self.label_sums(labels, row_labels, row0, nrows)
        return _means(s, counts).astype(np.float32), counts

    def kmeans(self, c: int, iterations: int = 10, seed: int = 0, init=None, spherical: bool = True,
               write_labels: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """k-means over the stored rows, every step on the device: per iteration one ``assign`` (the nearest centroid of
        every row by dot product) and one ``label_sums(arange(c), row_labels=best)`` (the update) -- c x D numbers and 4
        bytes per row cross PCIe, no row leaves HBM.  ``init`` (c, D): the first centroids; None: the stored values of
        ``c`` distinct rows drawn with ``np.random.default_rng(seed)`` (a tombstoned row's values are still in HBM).  A
        centroid is its cluster's mean over the LIVE rows, with ``spherical`` normalised to unit length in f64, then
        cast to f32; a cluster without a live row, or whose sum has zero norm, keeps its previous centroid.  The loop
        stops after ``iterations`` updates or as soon as ``best`` no longer changes.  Returns ``(centroids f32 (c, D),
        best i32 (n,), scores f32 (n,), counts i64 (c,), iterations run)``: best and scores are the last assignment's
        (against the centroids before it), counts its live rows per cluster, the centroids that assignment's means;
        iterations run = the updates made.  ``write_labels``: one final ``assign(centroids, labels=arange(c))`` writes
        the label column, and best, scores and counts are then its answer.  The rows are those the index holds when the
        call begins: rows appended while it runs take no part and get no label.  More than ASSIGN_MAX_VECTORS clusters,
        or fewer than one, is a ValueError."""
        try:
            c, iterations = operator.index(c), operator.index(iterations)
        except TypeError:
            raise ValueError(f"c and iterations must be integers, got {c!r} and {iterations!r}") from None
        if c < 1 or c > ASSIGN_MAX_VECTORS:
            raise ValueError(f"k-means takes 1 to {ASSIGN_MAX_VECTORS} clusters, got {c}")
        if iterations < 1:
            raise ValueError(f"iterations must be >= 1, got {iterations}")
        # ONE row range for the whole loop: rows appended while it runs (another thread, another owner of the handle)
        # are not part of this clustering, and no call of the loop sees another range than the one before it
        row0, n, d = self._extent()
        if init is None:
            if c > n:
                raise ValueError(f"{c} clusters for {n} rows")
            cent = self._stored_rows_at(np.random.default_rng(seed).choice(n, size=c, replace=False))
        else:
            cent = np.array(init, dtype=np.float32)
            if cent.shape != (c, d):
                raise ValueError(f"init must have shape ({c}, {d}), got {cent.shape}")
        ids = np.arange(c, dtype=np.uint32)
        prev, ran = None, 0
        while ran < iterations:
            best, scores, counts = self.assign(cent, row0=row0, nrows=n)
            if prev is not None and np.array_equal(best, prev):
                break                # (cent already holds this assignment's means)
            s, counts = self.label_sums(ids, row_labels=best, row0=row0, nrows=n)
            cent = _centroids(s, counts, cent, spherical)
            prev = best
            ran += 1
        if write_labels:
            best, scores, counts = self.assign(cent, labels=ids, row0=row0, nrows=n)
        return cent, best, scores, counts, ran

    def _extent(self) -> Tuple[int, int, int]:
        """(row_offset, n, d) as the HANDLE holds them now."""
        info = _native.IndexInfo()
        _native.check(self._quick.svs_index_info(self._handle(), C.byref(info)))
        return int(info.row_offset), int(info.n), int(info.d)

    def _stored_rows_at(self, rows, gap: int = 64) -> np.ndarray:
        """``stored_rows`` of the listed LOCAL rows, in the order given: the rows are read in ascending order, and rows
        no more than ``gap`` apart share one read (a few thousand rows are cheaper than a second blocking call)."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        out = np.empty((len(rows), self.shape[1]), dtype=np.float32)
        order = np.argsort(rows, kind="stable")
        at = 0
        while at < len(order):
            end = at + 1
            while end < len(order) and rows[order[end]] - rows[order[end - 1]] <= gap:
                end += 1
            first = int(rows[order[at]])
            block = self.stored_rows(first, int(rows[order[end - 1]]) - first + 1)
            out[order[at:end]] = block[rows[order[at:end]] - first]
            at = end
        return out

    @staticmethod
    def diverse_fetch(n: int, fetch_k: Optional[int] = None) -> int:
        """How many candidates a diverse search of ``n`` results re-ranks: ``fetch_k``, or by default
        min(max(4 n, 32), DIVERSE_MAX_FETCH), raised to ``n`` where ``n`` is larger.  More than DIVERSE_MAX_FETCH
        (results or candidates) is a ValueError."""
        n = max(n, 0)
        if n > DIVERSE_MAX_FETCH:
            raise ValueError(f"a diverse search returns at most {DIVERSE_MAX_FETCH} rows, {n} were asked for")
        if fetch_k is None:
            return max(min(max(4 * n, 32), DIVERSE_MAX_FETCH), n)
        assert isinstance(fetch_k, int)
        if fetch_k > DIVERSE_MAX_FETCH:
            raise ValueError(f"a diverse search re-ranks at most {DIVERSE_MAX_FETCH} candidates, fetch_k is {fetch_k}")
        if n > 0 and fetch_k < n:
            raise ValueError(f"fetch_k ({fetch_k}) is smaller than n ({n})")
        return fetch_k

    def search_batch_diverse(self, queries: np.ndarray, n: int, fetch_k: Optional[int] = None,
                             lam: float = 0.5) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Maximal-marginal-relevance re-ranking on the device (svs_index_search_diverse): for each row of ``queries``
        (nq, D) the ``fetch_k`` best rows are the candidates (``diverse_fetch``: by default min(max(4 n, 32), 1024)), and
        ``n`` of them are picked greedily by ``lam * score - (1 - lam) * (largest stored-row similarity to a row already
        picked)``, starting from the best; an exact tie goes to the better-ranked candidate.  Returns
        (scores f32 (nq, count), rows i64 (nq, count), redundancy f32 (nq, count)) in PICK order, count = min(max(n, 0),
        fetch_k, live rows); redundancy is that largest similarity when the row was picked (-inf for the first).
        ``lam=1`` is ``search_batch``; ``lam`` outside [0, 1] or NaN, and ``n`` or ``fetch_k`` above 1024, are
        ValueErrors."""
        assert isinstance(n, int)
        q = self._queries_2d(queries)
        nq, d = q.shape
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lam must lie in [0, 1], got {lam}")
        fk = self.diverse_fetch(n, fetch_k)
        h = self._pinned_handle()
        try:
            k = min(max(n, 0), max(fk, 0), self._live_rows(h))
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            red = np.empty((nq, k), dtype=np.float32)
            count = C.c_int32(0)
            # (the one call that releases the GIL)
            _native.check(self._lib.svs_index_search_diverse(h, q.ctypes.data, nq, d, k, fk, lam, scores.ctypes.data,
                                                             rows.ctypes.data, red.ctypes.data, C.byref(count)))
        finally:
            self._unpin(h)
        c = count.value
        return (scores, rows, red) if c == k else (scores[:, :c], rows[:, :c], red[:, :c])

    def search_diverse(self, query_vec: np.ndarray, n: int, fetch_k: Optional[int] = None,
                       lam: float = 0.5) -> List[Tuple[float, int, float]]:
        """``search`` re-ranked for diversity (see ``search_batch_diverse``): [(score, row, redundancy)] in pick order."""
        assert isinstance(n, int)
        q = _query_1d(query_vec)
        s, r, red = self.search_batch_diverse(q[None, :], n, fetch_k, lam)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist(), red[0].astype(np.float64).tolist()))

    def search_batch_combined(self, vectors: np.ndarray, n: int, op: str = "max",
                              weights=None) -> Tuple[np.ndarray, np.ndarray, int]:
        """Top-n of each COMBINED query (svs_index_search_combined): ``vectors`` is (nq, m, D), 1 <= m <= 8, and a row's
        score is the ``op`` -- "max", "min" or "sum" -- over its m terms ``weights[q, j] * scores(vectors[q, j])[row]``
        (``weights`` (nq, m), finite; None: every weight 1).  "max" and "min" compare in the order's own key (-0.0 equals
        +0.0, a NaN is the largest), "sum" adds the f32 terms in vector order.  One pass over the corpus and one
        selection per combined query, on the device.  Returns (scores f32 (nq, count), rows i64 (nq, count), count),
        count = min(max(n, 0), live rows), each row ordered (score desc, row desc); with m = 1, "max" and no weights
        that is ``search_batch`` on an unscreened index.  Shape, op and weight errors are ValueErrors."""
        assert isinstance(n, int)
        v, w = _combined_batch(vectors, op, weights)
        nq, m, d = v.shape
        h = self._pinned_handle()
        try:
            k = min(max(n, 0), self._live_rows(h))   # (clamped before allocating and before the int32 argument, as in search_batch)
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            count = C.c_int32(0)
            # (the one call that releases the GIL)
            _native.check(self._lib.svs_index_search_combined(h, v.ctypes.data, nq, m, d, None if w is None else w.ctypes.data,
                                                              COMBINE_OPS[op], k, scores.ctypes.data, rows.ctypes.data, C.byref(count)))
        finally:
            self._unpin(h)
        s, r = self._trimmed(scores, rows, count.value)
        return s, r, count.value

    def search_combined(self, vectors: np.ndarray, n: int, op: str = "max", weights=None) -> List[Tuple[float, int]]:
        """One combined query (see ``search_batch_combined``): ``vectors`` (m, D), ``weights`` (m,) or None;
        [(score, row)] as ``search`` returns them."""
        assert isinstance(n, int)
        v, w = _combined_one(vectors, weights)
        s, r, _ = self.search_batch_combined(v, n, op, w)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist()))

    def search_batch_collapsed_combined(self, vectors: np.ndarray, n: int, column: int, op: str = "max", weights=None,
                                        zero: str = "single") -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Group-combined search (svs_index_search_collapsed_combined): for each COMBINED query of ``vectors`` (nq, m,
        D) the ``n`` best groups of column ``column``, where a group's score against vector j is its BEST live row's
        and the m per-vector scores are combined as ``search_batch_combined`` combines a row's (``op``, ``weights``).
        A group is represented by the row ``search_batch_combined`` would rank first among its rows; ``zero`` as in
        ``search_batch_collapsed``.  Returns ``(scores f32 (nq, k), rows i64 (nq, k), values u32 (nq, k), counts i32
        (nq,), groups i64 (nq,))`` with k = min(max(n, 0), live rows): query i has counts[i] = min(k, groups[i]) valid
        entries; the entries past counts[i] are unspecified.  ``n=0`` only counts the groups."""
        assert isinstance(n, int)
        v, w = _combined_batch(vectors, op, weights)
        nq, m, d = v.shape
        c = column_index(column)
        mode = collapse_zero_mode(zero)
        h = self._pinned_handle()
        try:
            k = min(max(n, 0), self._live_rows(h))   # (clamped before allocating and before the int32 argument, as in search_batch)
            scores = np.empty((nq, k), dtype=np.float32)
            rows = np.empty((nq, k), dtype=np.int64)
            values = np.empty((nq, k), dtype=np.uint32)
            counts = np.zeros(nq, dtype=np.int32)
            groups = np.zeros(nq, dtype=np.int64)
            # (the one call that releases the GIL; a count-only call passes no result buffers)
            _native.check(self._lib.svs_index_search_collapsed_combined(
                h, v.ctypes.data, nq, m, d, None if w is None else w.ctypes.data, COMBINE_OPS[op], k, c, mode,
                scores.ctypes.data if k else None, rows.ctypes.data if k else None, values.ctypes.data if k else None,
                counts.ctypes.data, groups.ctypes.data))
        finally:
            self._unpin(h)
        return scores, rows, values, counts, groups

    def search_collapsed_combined(self, vectors: np.ndarray, n: int, column: int, op: str = "max", weights=None,
                                  zero: str = "single") -> Tuple[List[Tuple[float, int, int]], int]:
        """One group-combined query (see ``search_batch_collapsed_combined``): ``vectors`` (m, D), ``weights`` (m,) or
        None; ([(score, representative row, value)], groups), best group first."""
        assert isinstance(n, int)
        v, w = _combined_one(vectors, weights)
        s, r, val, counts, groups = self.search_batch_collapsed_combined(v, n, column, op, w, zero)
        c = int(counts[0])
        return list(zip(s[0, :c].astype(np.float64).tolist(), r[0, :c].tolist(), val[0, :c].tolist())), int(groups[0])

    def neighbors(self, rows, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """The ``n`` nearest stored rows of each listed stored row (GLOBAL indices, any order, repeats allowed), the
        row itself excluded: (scores f32 (len(rows), count), rows i64 (len(rows), count)), count = min(max(n, 0),
        live rows - 1), each row ordered (score desc, row desc) -- ``get_top_k(np.dot(M, M[r]), n + 1)`` without
        r, for every r, on the device (svs_index_neighbors).  A tombstoned or out-of-range row is a ValueError."""
        assert isinstance(n, int)
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        h = self._pinned_handle()
        try:
            # (clamped before allocating and before the int32 argument, as in search_batch)
            k = min(max(n, 0), max(self._live_rows(h) - 1, 0))
            scores = np.empty((len(r), k), dtype=np.float32)
            out_rows = np.empty((len(r), k), dtype=np.int64)
            count = C.c_int32(0)
            # (the one call that releases the GIL)
            _native.check(self._lib.svs_index_neighbors(h, r.ctypes.data, len(r), k, scores.ctypes.data, out_rows.ctypes.data,
                                                        C.byref(count)))
        finally:
            self._unpin(h)
        return self._trimmed(scores, out_rows, count.value)

    def scores(self, query_vec: np.ndarray) -> np.ndarray:
        """The raw ``np.dot(M, q)`` vector, f32 (N,)."""
        q = _query_1d(np.ascontiguousarray(query_vec, dtype=np.float32))
        h = self._pinned_handle()
        try:
            # The library writes one f32 per row the HANDLE holds when the call runs, never more than the capacity
            # passed: if rows were appended (another thread, another owner of the handle) since the buffer was
            # sized, the call fails, reports the new count, and is repeated with a buffer of that size.
            rows = self.n
            for _ in range(8):
                out = np.empty(rows, dtype=np.float32)
                now = C.c_int64(0)
                rc = self._lib.svs_index_scores_n(h, q.ctypes.data_as(C.c_void_p), q.shape[0],
                                                  out.ctypes.data_as(C.c_void_p), rows, C.byref(now))
                if rc == _native.SVS_OK:
                    return out[:now.value]
                if now.value <= rows:
                    break
                rows = now.value
            _native.check(rc)
            raise RuntimeError("svs_index_scores_n: the index kept growing")
        finally:
            self._unpin(h)

    def search_device(self, q_ptr: int, nq: int, d: int, k: int, out_scores_ptr: int,
                      out_rows_ptr: int, stream: int = 0) -> int:
        """Device-pointer variant (no synchronisation): see svs_index_search_device."""
        count = C.c_int32(0)
        h = self._pinned_handle()
        try:
            _native.check(self._lib.svs_index_search_device(
                h, C.c_void_p(q_ptr), int(nq), int(d), int(k), C.c_void_p(out_scores_ptr),
                C.c_void_p(out_rows_ptr), C.byref(count), C.c_void_p(stream)))
        finally:
            self._unpin(h)
        return count.value

    def search_device_ahead(self, q_ptr: int, nq: int, d: int, k: int, out_scores_ptr: int,
                            out_rows_ptr: int, stream: int = 0, ready_event=None) -> int:
        """``search_device`` for back-to-back single queries: the score pass runs on the library's own stream,
        beside the selection kernels of the search before it; results are ordered on ``stream`` as usual.  The
        query is NOT ordered by ``stream``: it must be complete on the device at the call, or ``ready_event`` (a
        raw hipEvent_t, or a ``torch.cuda.Event`` that HAS BEEN RECORDED) fires when it is; an event object without
        a handle yet (never recorded) is a ValueError, not an unguarded search.  See svs_index_search_device_ahead."""
        ev = getattr(ready_event, "cuda_event", ready_event)
        ev = getattr(ev, "value", ev)
        if ready_event is not None and not ev:
            raise ValueError("ready_event has no device handle: record it before passing it (an unrecorded event guards nothing)")
        count = C.c_int32(0)
        h = self._pinned_handle()
        try:
            _native.check(self._lib.svs_index_search_device_ahead(
                h, C.c_void_p(q_ptr), int(nq), int(d), int(k), C.c_void_p(out_scores_ptr),
                C.c_void_p(out_rows_ptr), C.byref(count), C.c_void_p(stream), C.c_void_p(ev or None)))
        finally:
            self._unpin(h)
        return count.value

    def top_pairs(self, n: int) -> List[Tuple[float, int, int]]:
        """``get_top_pairs(np.dot(M, M.T), n)`` (reference src/svs/kb.py:1651,
        src/svs/util.py:206-233): [(score, row_i, row_j)] with i < j."""
        assert isinstance(n, int)
        live = self._live_rows()
        k = min(max(n, 0), live * (live - 1) // 2)   # reference src/svs/util.py:198-199 on the pair list
        scores = np.empty(k, dtype=np.float32)
        ri = np.empty(k, dtype=np.int64)
        rj = np.empty(k, dtype=np.int64)
        count = C.c_int32(0)
        h = self._pinned_handle()
        try:
            _native.check(self._lib.svs_index_top_pairs(
                h, k, scores.ctypes.data_as(C.c_void_p), ri.ctypes.data_as(C.c_void_p),
                rj.ctypes.data_as(C.c_void_p), C.byref(count)))
        finally:
            self._unpin(h)
        c = count.value
        return [(float(s), int(a), int(b)) for s, a, b in zip(scores[:c], ri[:c], rj[:c])]

    # -- parity support -----------------------------------------------------
    def stored_rows(self, row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        """Rows exactly as held in HBM, dequantised to f32 (the corpus the oracle
        must be run on for the f16 / fp8 dtypes)."""
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty((nrows, self.d), dtype=np.float32)
        _native.check(self._lib.svs_index_debug_dequant(self._handle(), int(row0), int(nrows),
                                                        out.ctypes.data_as(C.c_void_p)))
        return out

    def stored_query(self, query_vec: np.ndarray) -> np.ndarray:
        """The query as this index's kernels see it (rounded / quantised)."""
        q = np.ascontiguousarray(query_vec, dtype=np.float32)
        out = np.empty_like(q)
        _native.check(self._lib.svs_index_debug_query(self._handle(), q.ctypes.data_as(C.c_void_p), q.shape[0],
                                                      out.ctypes.data_as(C.c_void_p)))
        return out

    # -- measurement ------------------------------------------------------
    def set_timing(self, enable) -> None:
        """True / 1: time every search; N: every N-th; False / 0: off."""
        _native.check(self._lib.svs_index_set_timing(self._handle(), int(enable)))

    def get_timing(self) -> Tuple[float, float, int]:
        t = _native.Timing()
        _native.check(self._lib.svs_index_get_timing(self._handle(), C.byref(t)))
        self.last_dominant_ms_sum = float(t.dominant_ms_sum)   # the dominant kernel alone (bench.py's roofline)
        return float(t.score_ms_sum), float(t.select_ms_sum), int(t.launches)

    def set_coalesce(self, enable: bool) -> None:
        """Concurrent single-query searches on this handle share corpus passes (svs_index_set_coalesce)."""
        _native.check(self._lib.svs_index_set_coalesce(self._handle(), 1 if enable else 0))

    def coalesce_stats(self) -> Tuple[int, int]:
        """(corpus passes, queries answered) through the coalescing path."""
        p, q = C.c_int64(0), C.c_int64(0)
        _native.check(self._lib.svs_index_coalesce_stats(self._handle(), C.byref(p), C.byref(q)))
        return p.value, q.value

    def coalesce_hold(self, n: int) -> None:
        """The next coalesced pass waits (at most 5 s) for n queued callers (svs_internal_coalesce_hold; tests)."""
        _native.check(self._lib.svs_internal_coalesce_hold(self._handle(), int(n)))

    def coalesce_sizes(self) -> dict:
        """{queries per pass: passes} of the coalescing path (svs_index_coalesce_sizes)."""
        out = (C.c_int64 * 257)()
        _native.check(self._lib.svs_index_coalesce_sizes(self._handle(), out, 257))
        return {s: int(out[s]) for s in range(257) if out[s]}

    def set_variant(self, variant: int) -> None:
        _native.check(self._lib.svs_index_set_variant(self._handle(), int(variant)))

    def set_screen(self, mode: int) -> None:
        """0: free the half shadow of an f32 index, every search reads the f32 rows; 1 (the default): keep it
        (+50 % HBM) and screen single queries on it -- same rows, order and score bits (svs_index_set_screen)."""
        _native.check(self._lib.svs_index_set_screen(self._handle(), int(mode)))
        self._refresh()

    def ahead_stats(self, shared: bool = False) -> dict:
        """``search_device_ahead`` on this handle (svs_internal_ahead_stats; tests): single-query calls that went through
        a pipeline, those that were plain calls because every pipeline had work in flight, idle pipelines handed over to
        another stream, pipelines that exist; then what those calls put on their pass streams: passes whose completion
        event their last kernel carried, event records, waits for a selection.

        ``shared=True`` adds the shared passes' counters (written by the claim kernels; drain the stream first):
        ``shared_passes`` that served more than one search, searches ``claimed`` by the pass of an earlier search, and
        ``empty_passes`` that found their search served already; ``thin_passes`` launched on the thin grid because
        the host expected them to be empty, ``thin_worked`` among them that had work after all, and ``thin_grid``, the
        workgroups of such a grid for this index's row length (0: its passes are never shared)."""
        out = (C.c_int64 * 13)()
        _native.check(self._lib.svs_internal_ahead_stats(self._handle(), out, 13))
        stats = {"ahead": int(out[0]), "plain": int(out[1]), "handed_over": int(out[2]), "pipelines": int(out[3]),
                 "bound": int(out[4]), "pass_records": int(out[5]), "pass_waits": int(out[6])}
        if shared:
            stats.update(shared_passes=int(out[7]), claimed=int(out[8]), empty_passes=int(out[9]),
                         thin_passes=int(out[10]), thin_worked=int(out[11]), thin_grid=int(out[12]))
        return stats

    def screen_stats(self) -> dict:
        """Counters and state of the screened search (svs_internal_screen_stats; tests).  Drain the stream first."""
        out = (C.c_int64 * 9)()
        _native.check(self._lib.svs_internal_screen_stats(self._handle(), out, 9))
        f = lambda b: float(np.array([b], dtype=np.uint32).view(np.float32)[0])
        return {"screened": int(out[0]), "fallback": int(out[1]), "shadow": int(out[2]), "paused": bool(out[3]),
                "E": f(out[4]), "n_cand": int(out[5]), "A": f(out[6]), "B": f(out[7]), "C": f(out[8])}

    def stored_image(self, what: str = "rows", row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        """Rows [row0, row0 + nrows) of an image byte for byte as it lies in HBM, copied without any kernel
        (svs_internal_stored_image; tests).  ``"rows"``: u8 (nrows, ld * element bytes), the padding columns included;
        ``"scales"``: f32 (nrows,), fp8 only; ``"shadow"``: u16 (nrows, ld), the half shadow of an f32 index.
        NotImplementedError when the index has no such image."""
        which = {"rows": 0, "scales": 1, "shadow": 2}[what]
        nrows = self.n - row0 if nrows is None else nrows
        if which == 0:
            out = np.empty((max(nrows, 0), self.ld * {"f32": 4, "f16": 2, "fp8": 1}[self.dtype]), dtype=np.uint8)
        elif which == 1:
            out = np.empty(max(nrows, 0), dtype=np.float32)
        else:
            out = np.empty((max(nrows, 0), self.ld), dtype=np.uint16)
        _native.check(self._lib.svs_internal_stored_image(self._handle(), which, int(row0), int(nrows),
                                                          out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # -- the top-k stage alone on caller-given data (svs_amd/csrc/internal.h; tests) ----------------
    def select_scores(self, scores: np.ndarray, k: int, row_offset: int = 0) -> Tuple[np.ndarray, np.ndarray, int, int]:
        """run_select over host ``scores`` (nq, n): (scores f32 (nq, k), rows i64 (nq, k), count, dirty scratch words)
        (svs_internal_select_scores).  Test hook; not part of the API."""
        s = np.ascontiguousarray(scores, dtype=np.float32)
        nq, n = s.shape
        out_s, out_r = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
        count, dirty = C.c_int32(0), C.c_int64(-1)
        _native.check(self._lib.svs_internal_select_scores(self._handle(), s.ctypes.data, nq, n, int(k), int(row_offset),
                                                           out_s.ctypes.data, out_r.ctypes.data, C.byref(count), C.byref(dirty)))
        return out_s, out_r, count.value, dirty.value

    def kth_value(self, scores: np.ndarray, k: int, misalign: bool = False) -> Tuple[np.ndarray, int]:
        """prefix_kth_kernel over host ``scores`` (nq, n): (k-th best score of every row f32 (nq,), dirty scratch words)
        (svs_internal_kth_value).  Test hook; not part of the API."""
        s = np.ascontiguousarray(scores, dtype=np.float32)
        nq, n = s.shape
        thr = np.empty(nq, dtype=np.float32)
        dirty = C.c_int64(-1)
        _native.check(self._lib.svs_internal_kth_value(self._handle(), s.ctypes.data, nq, n, int(k), int(bool(misalign)),
                                                       thr.ctypes.data, C.byref(dirty)))
        return thr, dirty.value

    def select_candidates(self, lists, claims, k: int, count: int, use_dead: bool = False) -> Tuple[np.ndarray, np.ndarray, int]:
        """select_final_kernel over per-query candidate key lists (u64: score key << 32 | local row, uploaded in the order
        given) whose headers claim ``claims[q]`` candidates: (scores f32 (nq, k), rows i64 (nq, k), dirty scratch words);
        a query the kernel could not answer has -2 in every row entry (svs_internal_select_candidates).  Test hook; not part of the API."""
        lists = [np.ascontiguousarray(x, dtype=np.uint64) for x in lists]
        nq = len(lists)
        offs = np.zeros(nq + 1, dtype=np.int64)
        offs[1:] = np.cumsum([x.size for x in lists])
        keys = np.concatenate(lists + [np.zeros(1, dtype=np.uint64)])   # (never empty: a pointer to pass)
        n_cand = np.ascontiguousarray(claims, dtype=np.uint32)
        assert n_cand.shape == (nq,)
        out_s, out_r = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
        dirty = C.c_int64(-1)
        _native.check(self._lib.svs_internal_select_candidates(self._handle(), keys.ctypes.data, offs.ctypes.data, n_cand.ctypes.data,
                                                               nq, int(k), int(count), int(bool(use_dead)), out_s.ctypes.data,
                                                               out_r.ctypes.data, C.byref(dirty)))
        return out_s, out_r, dirty.value

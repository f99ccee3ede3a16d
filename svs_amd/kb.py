"""
Host-side mirror of the reference's ``KB`` / ``AsyncKB`` **for the retrieve()
path only** (SURVEY.md section 8(a) rows A1, A6, A7, A8).

The reference's Python files do not travel to the GPU box, so this module gives
the parity tests (and users without the reference installed) the same surface:
``KB(path, embedding_func)``, ``bulk_add_docs()``, ``bulk_del_docs()``,
``retrieve(query, n) -> List[Retrieval]``, ``close()``, ``len()`` -- same
names, argument meaning and error behaviour as reference src/svs/kb.py:1407-1640
(sync) and :925-1206 (async).  Storage is a plain SQLite file with the
reference's schema v1 table layout (src/svs/kb.py:64-113), so a database
written by either implementation opens in the other; the graph / key-value /
hierarchy features of the reference are NOT rebuilt (out of scope, pure SQL).

The similarity search itself (``superheavy()``, src/svs/kb.py:1622-1627) is
``DeviceEmbeddingsMatrix.search`` -> HIP.  There is no numpy fallback.
"""
from __future__ import annotations

import asyncio
import json
import logging
import sqlite3
import struct
import sys
import threading
from contextlib import asynccontextmanager, contextmanager
from typing import Any, Awaitable, Callable, Dict, Iterator, List, Optional, Tuple

import numpy as np

from .index import ASSIGN_MAX_VECTORS, COMBINE_MAX_VECTORS, LABELS_MAX_SET, DeviceIndex
from .matrix import (DeviceEmbeddingsMatrix, above_op, assign_op, batch_op, by_label_op, cluster_op, collapsed_combined_op, collapsed_op, collapsed_where_op, combined_op, diverse_op, labeled_op, neighbors_op, pairs_op, segments_op, single_op, where_op,
                     within_op)

_LOG = logging.getLogger(__name__)

EmbeddingFunc = Callable[[List[str]], Awaitable[List[List[float]]]]   # reference src/svs/types.py:12

EMBEDDING_MAGNITUDE_TOLERANCE = 0.001   # reference src/svs/kb.py:58
BULK_EMBEDDING_CHUNK_SIZE = 200         # reference src/svs/kb.py:52
SCHEMA_VERSION = 1                      # reference src/svs/kb.py:61

# Table layout of the reference's schema v1 (data format, src/svs/kb.py:64-113).
_SCHEMA = [
    "CREATE TABLE IF NOT EXISTS keyval (id INTEGER PRIMARY KEY, key TEXT NOT NULL UNIQUE, val ANY NOT NULL) STRICT",
    "CREATE TABLE IF NOT EXISTS keyval_user (id INTEGER PRIMARY KEY, key TEXT NOT NULL UNIQUE, val ANY NOT NULL) STRICT",
    "CREATE TABLE IF NOT EXISTS embeddings (id INTEGER PRIMARY KEY, embedding BLOB NOT NULL) STRICT",
    "CREATE TABLE IF NOT EXISTS docs (id INTEGER PRIMARY KEY, parent_id INTEGER REFERENCES docs(id), "
    "level INTEGER NOT NULL, text TEXT NOT NULL, embedding INTEGER REFERENCES embeddings(id), meta TEXT) STRICT",
    "CREATE INDEX IF NOT EXISTS idx_docs_parent_id ON docs(parent_id)",
    "CREATE INDEX IF NOT EXISTS idx_docs_level ON docs(level)",
    "CREATE INDEX IF NOT EXISTS idx_docs_embedding ON docs(embedding)",
    "CREATE TABLE IF NOT EXISTS edges (id INTEGER PRIMARY KEY, a INTEGER REFERENCES docs(id) NOT NULL, "
    "b INTEGER REFERENCES docs(id) NOT NULL, r INTEGER REFERENCES docs(id) NOT NULL, w REAL, d INTEGER NOT NULL) STRICT",
    "CREATE UNIQUE INDEX IF NOT EXISTS idx_edges_abr ON edges(a, b, r)",
    "CREATE INDEX IF NOT EXISTS idx_edges_a ON edges(a)",
    "CREATE INDEX IF NOT EXISTS idx_edges_b ON edges(b)",
    "CREATE INDEX IF NOT EXISTS idx_edges_r ON edges(r)",
    "CREATE INDEX IF NOT EXISTS idx_edges_d ON edges(d)",
]


def embedding_to_bytes(embedding: List[float]) -> bytes:
    """Little-endian f32 BLOB codec, reference src/svs/embeddings/util.py:15-16."""
    return np.asarray(embedding, dtype="<f4").tobytes() if len(embedding) else b""


def embedding_from_bytes(blob: bytes) -> List[float]:
    """Reference src/svs/embeddings/util.py:19-23."""
    assert len(blob) % 4 == 0
    return [float(x) for x in np.frombuffer(blob, dtype="<f4")]


def check_magnitude(vectors: List[List[float]], tolerance: float = EMBEDDING_MAGNITUDE_TOLERANCE) -> None:
    """Unit-norm guard, reference src/svs/embeddings/util.py:34-39 (f32 norms).
    The HIP kernels compute a plain dot product and do NOT re-normalise, exactly
    like the reference, so this guard is what makes the score a cosine."""
    v = np.array(vectors, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError("embedding function must return a list of equal-length vectors")
    mags = np.sqrt((v * v).sum(axis=1))
    if (np.abs(mags - 1.0) > tolerance).any():
        raise ValueError("embedding magnitude out of spec")


class _Store:
    """Minimal SQLite access for the retrieve() path.  One connection, used from
    one thread at a time (callers serialise, as the reference does with its
    asyncio.Lock -- src/svs/kb.py:942-945)."""

    def __init__(self, path: str):
        self.path = str(path)
        self.conn = sqlite3.connect(self.path, isolation_level=None, check_same_thread=False)
        self.conn.execute("PRAGMA foreign_keys = ON")
        self._tx = threading.RLock()
        with self.transaction():
            for stmt in _SCHEMA:
                self.conn.execute(stmt)
            row = self.conn.execute("SELECT val FROM keyval WHERE key = 'schema_version'").fetchone()
            if row is None:
                self.conn.execute("INSERT INTO keyval (key, val) VALUES ('schema_version', ?)", (SCHEMA_VERSION,))
            elif row[0] != SCHEMA_VERSION:
                raise RuntimeError(f"unsupported schema version {row[0]}")

    @contextmanager
    def transaction(self):
        """All-or-nothing, like the reference's ``with db as q`` (src/svs/kb.py:806-817)."""
        with self._tx:
            self.conn.execute("BEGIN")
            try:
                yield self
            except BaseException:
                self.conn.execute("ROLLBACK")
                raise
            else:
                self.conn.execute("COMMIT")

    def close(self) -> None:
        self.conn.close()

    # -- docs ---------------------------------------------------------------
    def add_doc(self, text: str, parent_id: Optional[int], meta: Optional[Dict[str, Any]]) -> int:
        return self.add_doc_at(text, parent_id, meta)[0]

    def add_doc_at(self, text: str, parent_id: Optional[int], meta: Optional[Dict[str, Any]]) -> Tuple[int, int]:
        """``add_doc`` that also tells the level the doc landed on: (doc id, level)."""
        level = 0
        if parent_id is not None:
            row = self.conn.execute("SELECT level FROM docs WHERE id = ?", (parent_id,)).fetchone()
            if row is None:
                raise ValueError(f"invalid parent_id: {parent_id}")
            level = row[0] + 1
        cur = self.conn.execute(
            "INSERT INTO docs (parent_id, level, text, embedding, meta) VALUES (?, ?, ?, NULL, ?)",
            (parent_id, level, text, json.dumps(meta) if meta is not None else None))
        return int(cur.lastrowid), int(level)

    def set_doc_embedding(self, doc_id: int, blob: bytes) -> int:
        cur = self.conn.execute("INSERT INTO embeddings (embedding) VALUES (?)", (blob,))
        res = self.conn.execute("UPDATE docs SET embedding = ? WHERE id = ?", (cur.lastrowid, doc_id))
        if res.rowcount != 1:
            raise KeyError(doc_id)
        return int(cur.lastrowid)

    def del_doc(self, doc_id: int) -> Optional[int]:
        """Returns the id of the embedding that went with the document (if any)."""
        row = self.conn.execute("SELECT embedding FROM docs WHERE id = ?", (doc_id,)).fetchone()
        if row is None:
            raise KeyError(doc_id)
        self.conn.execute("DELETE FROM docs WHERE id = ?", (doc_id,))
        if row[0] is not None:
            self.conn.execute("DELETE FROM embeddings WHERE id = ?", (row[0],))
        return row[0]

    def count_docs(self) -> int:
        return int(self.conn.execute("SELECT COUNT(*) FROM docs").fetchone()[0])

    def fetch_doc_for_embedding(self, emb_id: int) -> Dict[str, Any]:
        """The two SELECTs per result of reference src/svs/kb.py:1633-1634, as one
        join; the record has the shape of fetch_doc(include_embedding=False)
        (src/svs/kb.py:464-473)."""
        row = self.conn.execute(
            "SELECT id, parent_id, level, text, embedding, meta FROM docs WHERE embedding = ?", (emb_id,)).fetchone()
        if row is None:
            raise KeyError(emb_id)
        return {"id": row[0], "parent_id": row[1], "level": row[2], "text": row[3],
                "embedding": row[4] is not None, "meta": json.loads(row[5]) if row[5] is not None else None}

    def fetch_docs_for_embeddings(self, emb_ids: List[int]) -> Dict[int, Dict[str, Any]]:
        """One ``IN (...)`` query for a whole result list (with
        the search on the GPU, the reference's 2 SELECTs per result become the
        bottleneck of ``retrieve()``)."""
        out: Dict[int, Dict[str, Any]] = {}
        for c0 in range(0, len(emb_ids), 500):   # stay under SQLITE_MAX_VARIABLE_NUMBER
            chunk = emb_ids[c0:c0 + 500]
            marks = ",".join("?" * len(chunk))
            for row in self.conn.execute(
                    f"SELECT id, parent_id, level, text, embedding, meta FROM docs WHERE embedding IN ({marks})", chunk):
                out[row[4]] = {"id": row[0], "parent_id": row[1], "level": row[2], "text": row[3],
                               "embedding": True, "meta": json.loads(row[5]) if row[5] is not None else None}
        return out

    def embeddings_for_docs(self, doc_ids: List[int]) -> List[int]:
        """Embedding ids of the listed docs, ascending and distinct (``retrieve_within``): one ``IN (...)``
        query per 500 ids, as ``fetch_docs_for_embeddings``.  An unknown doc id raises KeyError(doc_id),
        like the reference's fetch_doc; docs without an embedding are skipped."""
        ids = [int(x) for x in doc_ids]
        found: Dict[int, Optional[int]] = {}
        for c0 in range(0, len(ids), 500):   # stay under SQLITE_MAX_VARIABLE_NUMBER
            chunk = ids[c0:c0 + 500]
            marks = ",".join("?" * len(chunk))
            for row in self.conn.execute(f"SELECT id, embedding FROM docs WHERE id IN ({marks})", chunk):
                found[row[0]] = row[1]
        for doc_id in ids:
            if doc_id not in found:
                raise KeyError(doc_id)
        return sorted({e for e in found.values() if e is not None})

    def embedding_levels(self) -> Tuple[np.ndarray, np.ndarray]:
        """(embedding ids i64, labels u32) of every doc that has an embedding, in one scan (``retrieve_at_level``: the
        label column of the HBM copy).  The label of a doc is ``level + 1``: 0 is left for "not labelled yet"."""
        rows = self.conn.execute("SELECT embedding, level FROM docs WHERE embedding IS NOT NULL").fetchall()
        pairs = np.array(rows, dtype=np.int64).reshape(-1, 2)
        return pairs[:, 0].copy(), (pairs[:, 1] + 1).astype(np.uint32)

    def embedding_parents(self) -> Tuple[np.ndarray, np.ndarray]:
        """(embedding ids i64, values u32) of every doc that has an embedding, in one scan (``retrieve_under``: column
        ``PARENT_COLUMN`` of the HBM copy).  The value of a doc is ``parent_id + 1``; 0 means no parent.  ValueError for
        a stored parent id that does not fit (``_parent_value``)."""
        rows = self.conn.execute("SELECT embedding, parent_id FROM docs WHERE embedding IS NOT NULL").fetchall()
        ids = np.array([r[0] for r in rows], dtype=np.int64)
        return ids, np.array([_parent_value(r[1]) for r in rows], dtype=np.uint32)

    def embedded_levels(self) -> List[int]:
        """The distinct levels of the docs that have an embedding, ascending, in one statement
        (``retrieve_by_level`` with ``levels=None``)."""
        return [int(r[0]) for r in self.conn.execute("SELECT DISTINCT level FROM docs WHERE embedding IS NOT NULL ORDER BY level")]

    def embedding_of_doc(self, doc_id: int) -> int:
        """The embedding id of one doc (``retrieve_similar``): KeyError(doc_id) for an unknown doc, like the
        reference's fetch_doc; ValueError for a doc that was added without an embedding."""
        row = self.conn.execute("SELECT embedding FROM docs WHERE id = ?", (int(doc_id),)).fetchone()
        if row is None:
            raise KeyError(doc_id)
        if row[0] is None:
            raise ValueError(f"document {doc_id} has no embedding")
        return int(row[0])

    def docs_with_embeddings(self, doc_ids: Optional[List[int]] = None) -> List[Tuple[int, int]]:
        """[(doc_id, emb_id)] (``document_neighbors``).  None: every doc that has an embedding, in embedding-id
        order.  A list: those docs, in the order given; KeyError(doc_id) for an unknown doc, ValueError for one
        without an embedding."""
        if doc_ids is None:
            return [(int(r[0]), int(r[1])) for r in self.conn.execute(
                "SELECT id, embedding FROM docs WHERE embedding IS NOT NULL ORDER BY embedding")]
        ids = [int(x) for x in doc_ids]
        found: Dict[int, Optional[int]] = {}
        for c0 in range(0, len(ids), 500):   # stay under SQLITE_MAX_VARIABLE_NUMBER
            chunk = ids[c0:c0 + 500]
            marks = ",".join("?" * len(chunk))
            for row in self.conn.execute(f"SELECT id, embedding FROM docs WHERE id IN ({marks})", chunk):
                found[row[0]] = row[1]
        for doc_id in ids:
            if doc_id not in found:
                raise KeyError(doc_id)
            if found[doc_id] is None:
                raise ValueError(f"document {doc_id} has no embedding")
        return [(d, int(found[d])) for d in ids]

    def doc_ids_for_embeddings(self, emb_ids: Optional[List[int]] = None) -> Dict[int, int]:
        """{emb_id: doc_id}, ids only -- no text, no meta (``document_neighbors``: a 1M-doc graph names 100M
        neighbours).  None: one scan over every doc that has an embedding; a list: ``IN (...)`` per 500 ids."""
        if emb_ids is None:
            return {int(r[0]): int(r[1]) for r in self.conn.execute(
                "SELECT embedding, id FROM docs WHERE embedding IS NOT NULL")}
        out: Dict[int, int] = {}
        for c0 in range(0, len(emb_ids), 500):
            chunk = emb_ids[c0:c0 + 500]
            marks = ",".join("?" * len(chunk))
            for row in self.conn.execute(f"SELECT embedding, id FROM docs WHERE embedding IN ({marks})", chunk):
                out[int(row[0])] = int(row[1])
        return out

    # -- A7: the producer of the matrix ---------------------------------------
    def build_embeddings_matrix(self) -> Tuple[np.ndarray, np.ndarray]:
        """Same contract as reference src/svs/kb.py:573-618 -- f32 (n, m) C-contiguous
        matrix + i64 ids, rows in ``SELECT id, embedding FROM embeddings`` order, m
        from the first row, empty table -> shape (0, 0) -- but each BLOB (already
        little-endian f32, src/svs/embeddings/util.py:15-16) is byte-copied straight
        into its row through a memoryview instead of ``struct.unpack`` -> python list
        -> element-wise assign: 4.7 s instead of ~130 s per 1M rows on the build
        container (the reference's published 98.7 s cold start)."""
        n = int(self.conn.execute("SELECT COUNT(*) FROM embeddings").fetchone()[0])
        first = self.conn.execute("SELECT embedding FROM embeddings LIMIT 1").fetchone()
        m = len(first[0]) // 4 if first is not None else 0
        matrix = np.zeros((n, m), dtype=np.float32)
        lookup = np.zeros(n, dtype=np.int64)
        assert sys.byteorder == "little"   # the BLOB codec is '<f'; a big-endian host would need a byteswap
        raw = memoryview(matrix).cast("B") if n * m else None
        rb = m * 4
        i = -1
        for i, (emb_id, blob) in enumerate(self.conn.execute("SELECT id, embedding FROM embeddings")):
            assert len(blob) == rb
            if rb:
                raw[i * rb:(i + 1) * rb] = blob
            lookup[i] = emb_id
        assert i == n - 1
        return matrix, lookup

    def embedding_blocks(self, block_bytes: int = 32 << 20, acquire=None):
        """The same rows as ``build_embeddings_matrix`` without the (n, m) host matrix: yields
        (n, m) first, then (ids i64[r], rows f32[r, m]) blocks of ~32 MiB -- the size of the library's
        pinned staging chunks -- each BLOB byte-copied into the block through a memoryview.  The
        consumer appends every block to the HBM copy (svs_index_append) before asking for the next,
        so the host never holds more than one block of a 6 GB (1M x 1536) corpus.  The block buffer is
        reused: copy what you keep.  With ``acquire`` every block is decoded into the (cap, m) f32
        array that call returns (asked for again after each yield) instead of a private buffer."""
        n = int(self.conn.execute("SELECT COUNT(*) FROM embeddings").fetchone()[0])
        first = self.conn.execute("SELECT embedding FROM embeddings LIMIT 1").fetchone()
        m = len(first[0]) // 4 if first is not None else 0
        yield n, m
        if n * m == 0:
            return
        assert sys.byteorder == "little"
        rb = m * 4

        def fresh():
            b = acquire() if acquire is not None else np.empty((max(1, block_bytes // rb), m), dtype=np.float32)
            assert b.dtype == np.float32 and b.ndim == 2 and b.shape[1] == m and b.flags["C_CONTIGUOUS"]
            return b, memoryview(b).cast("B")

        buf, raw = fresh()
        cap = buf.shape[0]
        ids = np.empty(cap, dtype=np.int64)
        fill = total = 0
        for emb_id, blob in self.conn.execute("SELECT id, embedding FROM embeddings"):
            assert len(blob) == rb
            raw[fill * rb:(fill + 1) * rb] = blob
            ids[fill] = emb_id
            fill += 1
            if fill == cap:
                yield ids[:fill], buf[:fill]
                total += fill
                fill = 0
                if acquire is not None:      # the consumer has committed the block: take the other one
                    buf, raw = fresh()
                    assert buf.shape[0] == cap
        if fill:
            yield ids[:fill], buf[:fill]
            total += fill
        assert total == n


def _build_from_store(store: _Store) -> Tuple[np.ndarray, np.ndarray]:
    with store.transaction():
        return store.build_embeddings_matrix()


def _blocks_from_store(store: _Store, acquire=None):
    """Streaming form of the cold start: first (n, m), then (ids, rows)
    blocks in ``SELECT id, embedding FROM embeddings`` order, inside one read transaction.
    ``acquire()`` (optional) supplies the block to decode into -- the library's pinned staging
    memory (DeviceIndex.staging_acquire) -- so a BLOB's bytes are copied exactly once on the host."""
    with store.transaction():
        yield from store.embedding_blocks(acquire=acquire)


def _device_matrix(device: int, index_factory: Callable[..., Any], dtype: str) -> DeviceEmbeddingsMatrix:
    """The matrix cache of ``KB`` / ``AsyncKB``: built from the store, streamed, no host copy."""
    if dtype != "f32":   # storage dtype of the HBM copy ("f16", "fp8"); f32 is the reference's arithmetic
        import functools
        index_factory = functools.partial(index_factory, dtype=dtype)
    return DeviceEmbeddingsMatrix(device=device, builder=_build_from_store, index_factory=index_factory,
                                  keep_host_matrix=False, block_builder=_blocks_from_store)


def _chunks(texts: List[str]) -> List[List[str]]:
    """``texts`` in slices of ``BULK_EMBEDDING_CHUNK_SIZE`` (as it reads now), the way bulk_add_docs embeds."""
    return [texts[c0:c0 + BULK_EMBEDDING_CHUNK_SIZE] for c0 in range(0, len(texts), BULK_EMBEDDING_CHUNK_SIZE)]


def _fetch_list(db: _Store, emb_ids: List[Tuple[float, int]]) -> List[Dict[str, Any]]:
    """[(score, emb id)] -> ``Retrieval`` list, the docs fetched with one SQL statement; call it in a transaction."""
    docs = db.fetch_docs_for_embeddings([e for _, e in emb_ids])
    return [{"score": s, "doc": docs[e]} for s, e in emb_ids]


def _fetch_lists(db: _Store, per_list: List[List[Tuple[float, int]]]) -> List[List[Dict[str, Any]]]:
    """``_fetch_list`` of every list: one SQL fetch per list (as ``retrieve_many``)."""
    return [_fetch_list(db, emb_ids) for emb_ids in per_list]


def _fetch_diverse(db: _Store, picks: List[Tuple[float, int, float]]) -> List[Dict[str, Any]]:
    """[(score, emb id, redundancy)] in pick order -> ``Retrieval`` list with a 'redundancy' key, the docs fetched with
    one SQL statement; call it in a transaction."""
    docs = db.fetch_docs_for_embeddings([e for _, e, _ in picks])
    return [{"score": s, "doc": docs[e], "redundancy": r} for s, e, r in picks]


def _fetch_by_level(db: _Store, groups: List[Tuple[int, float, int, int]]) -> List[Dict[str, Any]]:
    """[(label, score, emb id, count)], best label first -> [{'level', 'count', 'score', 'doc'}] (the label of a level
    is ``level + 1``), the docs fetched with one SQL statement; call it in a transaction."""
    docs = db.fetch_docs_for_embeddings([e for _, _, e, _ in groups])
    return [{"level": label - 1, "count": count, "score": s, "doc": docs[e]} for label, s, e, count in groups]


def _by_level_cut(min_score: Optional[float]) -> Optional[float]:
    """The cut-off of ``retrieve_by_level`` as a float (None: every document); ValueError for a NaN."""
    if min_score is None:
        return None
    if min_score != min_score:
        raise ValueError("min_score is NaN")
    return float(min_score)


PARENT_COLUMN = 1   # the column of the HBM copy that holds parent_id + 1 (column 0: level + 1)


def _parent_value(parent_id) -> int:
    """What column ``PARENT_COLUMN`` holds for a doc: ``parent_id + 1``, and 0 for a doc without a parent.  ValueError
    for a parent id that is negative or no integer, or >= 2**32 - 1 (its value would not fit in a u32)."""
    if parent_id is None:
        return 0
    if isinstance(parent_id, (bool, np.bool_)) or not isinstance(parent_id, (int, np.integer)):
        raise ValueError(f"a parent id must be an integer, got {parent_id!r}")
    if parent_id < 0:
        raise ValueError(f"a parent id cannot be negative, got {parent_id}")
    if parent_id >= 0xFFFFFFFF:
        raise ValueError(f"parent id {parent_id} is too large: the column holds parent_id + 1 as a u32")
    return int(parent_id) + 1


def _parent_values(parent_ids) -> List[int]:
    """The set of ``retrieve_under``: ``parent_ids`` (an int or an iterable of ints) as the distinct stored values
    ``parent_id + 1``, ascending.  ValueError as ``_parent_value`` (None is no parent id here), and for more than
    ``LABELS_MAX_SET`` distinct parents."""
    if isinstance(parent_ids, (int, np.integer)) and not isinstance(parent_ids, bool):
        given = [parent_ids]
    elif isinstance(parent_ids, (str, bytes)) or not hasattr(parent_ids, "__iter__"):
        raise ValueError(f"parent_ids must be an integer or an iterable of integers, got {parent_ids!r}")
    else:
        given = list(parent_ids)
    if any(p is None for p in given):
        raise ValueError("a parent id must be an integer, got None")
    values = sorted({_parent_value(p) for p in given})
    if len(values) > LABELS_MAX_SET:
        raise ValueError(f"{len(values)} distinct parents; one retrieval names at most {LABELS_MAX_SET}")
    return values


def _parent_column(parent_ids) -> Optional[List[int]]:
    """Column ``PARENT_COLUMN``'s values of the rows a ``bulk_add_docs`` appends, or None when one of the parent ids
    does not fit: the append then leaves the column not installed, and the next ``retrieve_under`` meets the id in its
    scan of the store and raises there."""
    try:
        return [_parent_value(p) for p in parent_ids]
    except ValueError:
        return None


def _under_where(parent_ids, levels) -> list:
    """The predicate of ``retrieve_under``: a child of one of ``parent_ids``, and on one of ``levels`` unless None."""
    where = [(PARENT_COLUMN, "in", _parent_values(parent_ids))]
    if levels is not None:
        where.append((0, "in", _level_labels(levels)))
    return where


def _level_labels(levels) -> List[int]:
    """The label set of ``retrieve_at_level``: ``levels`` (an int or an iterable of ints) as the distinct stored labels
    ``level + 1``, ascending.  ValueError for a level that is negative or no integer, and for more than
    ``LABELS_MAX_SET`` distinct levels."""
    if isinstance(levels, (int, np.integer)):
        given = [levels]
    elif isinstance(levels, (str, bytes)) or not hasattr(levels, "__iter__"):
        raise ValueError(f"levels must be an integer or an iterable of integers, got {levels!r}")
    else:
        given = list(levels)
    for lv in given:
        if isinstance(lv, bool) or not isinstance(lv, (int, np.integer)):
            raise ValueError(f"a level must be an integer, got {lv!r}")
        if lv < 0:
            raise ValueError(f"a level cannot be negative, got {lv}")
        if lv + 1 > 0xFFFFFFFF:
            raise ValueError(f"level {lv} is too large")
    labels = sorted({int(lv) + 1 for lv in given})
    if len(labels) > LABELS_MAX_SET:
        raise ValueError(f"{len(labels)} distinct levels; one retrieval names at most {LABELS_MAX_SET}")
    return labels


def _classify_topics(topics: List[str]) -> List[str]:
    """The topics of ``classify_documents`` as a list; ValueError for none or more than ``ASSIGN_MAX_VECTORS``."""
    topics = list(topics)
    if not topics:
        raise ValueError("classify_documents needs at least one topic")
    if len(topics) > ASSIGN_MAX_VECTORS:
        raise ValueError(f"{len(topics)} topics; one classification takes at most {ASSIGN_MAX_VECTORS}")
    return topics


def _classified(assigned, doc_of: Dict[int, int], n_topics: int) -> Dict[str, np.ndarray]:
    """(emb ids, best, scores, counts) of ``DeviceEmbeddingsMatrix.assign`` -> {'doc_ids', 'topic', 'score', 'counts'};
    an embedding whose doc left the store since is dropped, and the counts are those of the docs returned."""
    emb_ids, best, scores, counts = assigned
    known = np.fromiter((int(e) in doc_of for e in emb_ids), dtype=bool, count=len(emb_ids))
    if not known.all():
        emb_ids, best, scores = emb_ids[known], best[known], scores[known]
        counts = np.bincount(best, minlength=n_topics).astype(np.int64)
    doc_ids = np.fromiter((doc_of[int(e)] for e in emb_ids), dtype=np.int64, count=len(emb_ids))
    return {"doc_ids": doc_ids, "topic": best.astype(np.int32), "score": scores.astype(np.float32),
            "counts": np.asarray(counts, dtype=np.int64)}


def _cluster_args(n_clusters: int, iterations: int) -> None:
    """ValueError for fewer than one or more than ``ASSIGN_MAX_VECTORS`` clusters, or fewer than one iteration."""
    if not 1 <= int(n_clusters) <= ASSIGN_MAX_VECTORS:
        raise ValueError(f"{n_clusters} clusters; one clustering takes 1 to {ASSIGN_MAX_VECTORS}")
    if int(iterations) < 1:
        raise ValueError(f"iterations must be >= 1, got {iterations}")


def _clustered(clustered, doc_of: Dict[int, int], n_clusters: int) -> Dict[str, Any]:
    """(emb ids, cluster, scores, counts, centroids, iterations) of ``DeviceEmbeddingsMatrix.cluster`` -> {'doc_ids',
    'cluster', 'score', 'counts', 'centroids', 'iterations'}; dropped docs and counts as in ``_classified``."""
    res = _classified(clustered[:4], doc_of, n_clusters)
    return {"doc_ids": res["doc_ids"], "cluster": res["topic"], "score": res["score"], "counts": res["counts"],
            "centroids": np.asarray(clustered[4], dtype=np.float32), "iterations": int(clustered[5])}


_COMBINED_MODES = {"any": "max", "all": "min", "sum": "sum"}


def _combined_args(queries: List[str], mode: str, weights) -> Tuple[List[str], str, Optional[np.ndarray]]:
    """(query strings, the index's op, weights f32 (m,) or None) of a combined retrieval; ValueError for no query or more
    than 8, an unknown mode, and weights that are not one finite number per query."""
    queries = list(queries)
    if not 1 <= len(queries) <= COMBINE_MAX_VECTORS:
        raise ValueError(f"a combined retrieval takes 1 .. {COMBINE_MAX_VECTORS} queries, got {len(queries)}")
    if mode not in _COMBINED_MODES:
        raise ValueError(f"mode must be one of {sorted(_COMBINED_MODES)}, got {mode!r}")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32)
        if w.shape != (len(queries),) or not np.isfinite(w).all():
            raise ValueError(f"weights must be {len(queries)} finite numbers, one per query")
    return queries, _COMBINED_MODES[mode], w


def _diverse_args(n: int, fetch_n: Optional[int], diversity: float) -> Tuple[int, float]:
    """(candidates to fetch, lambda_mult = 1 - diversity) of a diverse retrieval; ValueError for a diversity outside
    [0, 1] or NaN, more than 1024 results or candidates, or fewer candidates than results."""
    diversity = float(diversity)
    if not 0.0 <= diversity <= 1.0:
        raise ValueError(f"diversity must lie in [0, 1], got {diversity}")
    return DeviceIndex.diverse_fetch(n, fetch_n), 1.0 - diversity


class KB:
    """Sync knowledge base, retrieve() path only.  Mirrors reference
    src/svs/kb.py:1407-1640."""

    def __init__(self, local_path: str, embedding_func: Optional[EmbeddingFunc] = None,
                 device: int = 0, index_factory: Callable[..., Any] = DeviceIndex, dtype: str = "f32"):
        if embedding_func is None:
            raise RuntimeError("No embedding function. You must pass the embedding function you want to use.")
        self.embedding_func = embedding_func
        self.db: Optional[_Store] = _Store(local_path)
        self.embeddings_matrix = _device_matrix(device, index_factory, dtype)
        self._loop = asyncio.new_event_loop()

    # -- embedding helpers (A8) -------------------------------------------------
    def _embed(self, texts: List[str]) -> List[List[float]]:
        awaitable = self.embedding_func(texts)
        assert asyncio.iscoroutine(awaitable)
        vectors = self._loop.run_until_complete(awaitable)
        check_magnitude(vectors)
        return vectors

    def _embed_chunked(self, texts: List[str]) -> List[List[float]]:
        return [vec for chunk in _chunks(texts) for vec in self._embed(chunk)]

    def __len__(self) -> int:
        assert self.db is not None
        with self.db.transaction():
            return self.db.count_docs()

    def load(self) -> None:
        """Reference ``load()``: build the matrix now instead of at the first
        retrieve() (src/svs/kb.py:964-967 async twin)."""
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

    def close(self) -> None:
        if self.db is not None:
            self.db.close()
            self.db = None
            self.embeddings_matrix.invalidate()
        if not self._loop.is_closed():
            self._loop.close()

    @contextmanager
    def bulk_add_docs(self) -> Iterator[Callable[..., int]]:
        """Reference src/svs/kb.py:1486-1524: docs are inserted inside ONE
        transaction, embeddings are fetched in chunks of 200 at exit, then the
        cached matrix is invalidated."""
        assert self.db is not None
        new_ids: List[int] = []
        new_vecs: List[List[float]] = []
        new_labels: List[int] = []     # level + 1 of every new embedding's doc (retrieve_at_level)
        new_parents: List[Optional[int]] = []   # its parent id (retrieve_under)
        try:
            with self.db.transaction():
                live = True
                pending: List[Tuple[int, str, int, Optional[int]]] = []

                def add_doc(text: str, parent_id: Optional[int] = None, meta: Optional[Dict[str, Any]] = None,
                            no_embedding: bool = False) -> int:
                    assert live, "You may not call this function outside of the context manager!"
                    doc_id, level = self.db.add_doc_at(text, parent_id, meta)
                    if not no_embedding:
                        pending.append((doc_id, text, level, parent_id))
                    return doc_id

                try:
                    yield add_doc
                finally:
                    live = False
                for c0 in range(0, len(pending), BULK_EMBEDDING_CHUNK_SIZE):
                    chunk = pending[c0:c0 + BULK_EMBEDDING_CHUNK_SIZE]
                    vectors = self._embed([c[1] for c in chunk])
                    for (doc_id, _, level, parent_id), vec in zip(chunk, vectors):
                        new_ids.append(self.db.set_doc_embedding(doc_id, embedding_to_bytes(vec)))
                        new_vecs.append(vec)
                        new_labels.append(level + 1)
                        new_parents.append(parent_id)
        except BaseException:
            self.embeddings_matrix.invalidate()
            raise
        # committed: the reference drops the whole cached matrix here (kb.py:1523); the
        # HBM copy is instead extended in place (falls back to invalidate when not loaded)
        if new_ids:
            self.embeddings_matrix.append(np.array(new_vecs, dtype=np.float32), new_ids, labels=new_labels,
                                          columns={PARENT_COLUMN: _parent_column(new_parents)})

    @contextmanager
    def bulk_del_docs(self) -> Iterator[Callable[[int], None]]:
        """Reference src/svs/kb.py:1526-1542."""
        assert self.db is not None
        gone: List[int] = []
        try:
            with self.db.transaction():
                live = True

                def del_doc(doc_id: int) -> None:
                    assert live, "You may not call this function outside of the context manager!"
                    emb_id = self.db.del_doc(doc_id)
                    if emb_id is not None:
                        gone.append(emb_id)

                try:
                    yield del_doc
                finally:
                    live = False
        except BaseException:
            self.embeddings_matrix.invalidate()
            raise
        if gone:   # reference: invalidate() (kb.py:1541); here the rows are tombstoned in HBM
            self.embeddings_matrix.remove(gone)

    def retrieve(self, query: str, n: int) -> List[Dict[str, Any]]:
        """Reference src/svs/kb.py:1608-1640.  Same four log lines, same result
        shape (``Retrieval``: {'score': float, 'doc': DocumentRecord})."""
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        emb_ids = self.embeddings_matrix.search(query_vec, n)          # superheavy(): HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        with self.db.transaction():
            res = [{"score": score, "doc": self.db.fetch_doc_for_embedding(emb_id)} for score, emb_id in emb_ids]
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_within(self, query: str, n: int, doc_ids: List[int]) -> List[Dict[str, Any]]:
        """``retrieve`` restricted to the documents ``doc_ids`` (the children of one parent, the docs of one
        level, ...): the top n of those docs, same log lines and result shape.  Only their rows are scored
        (svs_index_search_rows).  An unknown doc id raises KeyError; docs without an embedding are skipped."""
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        with self.db.transaction():
            emb = self.db.embeddings_for_docs(list(doc_ids))
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        emb_ids = self.embeddings_matrix.search_within(query_vec, n, emb)   # superheavy() over the listed rows: HIP
        _LOG.info(f"computed {len(emb)} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_above(self, query: str, min_score: float, n: int) -> Tuple[List[Dict[str, Any]], int]:
        """Every document whose score is at or above ``min_score``, best first, at most ``n`` of them, and how many
        qualify in all: (``retrieve``-shaped list, total).  ``n=0`` only counts.  The cut is made on the device
        (svs_index_search_above): neither a guessed ``n`` nor the score vector crosses the bus.  A NaN cut-off
        raises ValueError."""
        if min_score != min_score:
            raise ValueError("min_score is NaN")
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        emb_ids, total = self.embeddings_matrix.search_above(query_vec, float(min_score), n)   # HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res, total

    def retrieve_at_level(self, query: str, n: int, levels) -> List[Dict[str, Any]]:
        """``retrieve`` restricted to the documents of one level of the tree (``levels``: an int) or of several (an
        iterable of ints): the top n of those docs, same log lines and result shape.  The level sits next to each
        vector in HBM as a label (``level + 1``; 0 = not labelled yet, which matches no level) and the filter runs on
        the device (svs_index_search_labeled): no doc-id list, no SQL per query.  The column is installed at the first
        such retrieval of an index generation, by one scan of the docs table; afterwards ``bulk_add_docs`` labels the
        rows it appends and deletions move the labels with the rows.  A level no doc has gives ``[]``; a negative
        level, or more than 1,024 distinct ones, raises ValueError.  A doc added concurrently becomes visible here when
        its label is set, a moment after ``retrieve`` sees it."""
        labels = _level_labels(levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

        def levels_from_store():
            with self.db.transaction():
                return self.db.embedding_levels()

        self.embeddings_matrix.ensure_labels(levels_from_store)
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        emb_ids, matched = self.embeddings_matrix.search_labeled(query_vec, n, labels)   # filter + superheavy(): HIP
        _LOG.info(f"computed {matched} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_under(self, query: str, n: int, parent_ids, levels=None) -> List[Dict[str, Any]]:
        """``retrieve`` restricted to the children of ``parent_ids`` (an int or an iterable of ints, at most 1,024
        distinct), and with ``levels`` also to those levels as in ``retrieve_at_level``: the top n of those docs, same
        log lines and result shape -- the answer of ``retrieve_within`` over those children's ids.  ``parent_id + 1``
        sits next to each vector in HBM in column ``PARENT_COLUMN`` (0 = no parent) beside the level in column 0, and
        the conjunction runs on the device (svs_index_search_where): no doc-id list, no SQL per query.  The column is
        installed and maintained exactly like the level column: at the first such retrieval of an index generation,
        by one scan of the docs table; afterwards ``bulk_add_docs`` passes the values of the rows it appends and
        deletions move them with the rows.  No parent, or a parent without children, gives ``[]``; a parent id that is
        negative, no integer or >= 2**32 - 1, in the call or in the store, raises ValueError."""
        where = _under_where(parent_ids, levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

        def from_store(read):
            def fetch():
                with self.db.transaction():
                    return read()
            return fetch

        self.embeddings_matrix.ensure_column(PARENT_COLUMN, from_store(self.db.embedding_parents))
        if levels is not None:
            self.embeddings_matrix.ensure_labels(from_store(self.db.embedding_levels))
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        emb_ids, matched = self.embeddings_matrix.search_where(query_vec, n, where)   # filter + superheavy(): HIP
        _LOG.info(f"computed {matched} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_collapsed(self, query: str, n: int, levels=None) -> List[Dict[str, Any]]:
        """``retrieve`` with at most ONE document per parent: the n best documents after every parent's children are
        represented by the best of them -- "the 10 best sections, one per chapter" -- same log lines and result shape.
        A document without a parent stands for itself.  ``parent_id + 1`` sits next to each vector in HBM in column
        ``PARENT_COLUMN`` (0 = no parent), the column ``retrieve_under`` installs and maintains, and the grouping runs
        on the device in the query's one corpus pass (svs_index_search_collapsed): no over-fetching, and a parent that
        holds the best 500 documents still yields one.
        Without ``levels`` every level of the tree is grouped at once: a root stands for itself, its children are one
        group and each child's children another, so one subtree can take several places.  ``levels`` (an int or an
        iterable of ints as in ``retrieve_at_level``) keeps the search inside those levels: only their documents are
        scored, and a parent is represented by its best child THERE (svs_index_search_collapsed_where over the level
        column and the parent column); the third log line then counts the documents of those levels.  A level no
        document has gives ``[]``."""
        labels = None if levels is None else _level_labels(levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

        def from_store(read):
            def fetch():
                with self.db.transaction():
                    return read()
            return fetch

        self.embeddings_matrix.ensure_column(PARENT_COLUMN, from_store(self.db.embedding_parents))
        if labels is not None:
            self.embeddings_matrix.ensure_labels(from_store(self.db.embedding_levels))
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        if labels is None:
            hits, _ = self.embeddings_matrix.search_collapsed(query_vec, n, PARENT_COLUMN, "single")   # one pass + grouping: HIP
            _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        else:
            hits, _, matched = self.embeddings_matrix.search_collapsed_where(query_vec, n, [(0, "in", labels)], PARENT_COLUMN,
                                                                             "single")   # filter + gather + grouping: HIP
            _LOG.info(f"computed {matched} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, [(score, emb_id) for score, emb_id, _ in hits])
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_by_level(self, query: str, min_score: Optional[float] = None, levels=None) -> List[Dict[str, Any]]:
        """The breakdown of one query over the levels of the tree: for every level that has a document scoring at or
        above ``min_score`` (None: any document) the best such document and how many there are --
        [{'level': int, 'count': int, 'score': float, 'doc': DocumentRecord}], best level first.  ``levels``: an int or
        an iterable of ints as in ``retrieve_at_level``; None: every level present in the store.  One corpus pass on
        the device whatever the number of levels (svs_index_search_by_label) over the label column
        ``retrieve_at_level`` uses; a level nobody has, or none of whose documents reaches the cut-off, is absent.  A
        NaN cut-off, a negative level, or more than 1,024 distinct levels raises ValueError."""
        cut = _by_level_cut(min_score)
        labels = None if levels is None else _level_labels(levels)
        _LOG.info(f"retrieving the best document of {'every level' if labels is None else f'{len(labels)} levels'} with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

        def levels_from_store():
            with self.db.transaction():
                return self.db.embedding_levels()

        self.embeddings_matrix.ensure_labels(levels_from_store)
        if labels is None:
            with self.db.transaction():
                labels = _level_labels(self.db.embedded_levels())
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        groups = self.embeddings_matrix.search_by_label(query_vec, labels, cut) if labels else []   # one pass + reduction: HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        with self.db.transaction():
            res = _fetch_by_level(self.db, groups)
        _LOG.info(f"retrieved the best documents of {len(res)} levels")
        return res

    def classify_documents(self, topics: List[str]) -> Dict[str, np.ndarray]:
        """Zero-shot tagging: every document that has an embedding gets the topic its embedding scores best against.
        The topic strings are embedded like queries and the whole corpus is assigned in ONE native call on the device
        (svs_index_assign) -- nothing is pulled out of HBM but 8 bytes per document.  Returns {'doc_ids': int64 (m,),
        'topic': int32 (m,), 'score': float32 (m,), 'counts': int64 (len(topics),)}: ``topic[i]`` is the position in
        ``topics`` of document ``doc_ids[i]``'s best topic (an exact tie goes to the earlier topic), ``counts[t]`` the
        number of documents of topic t; documents in embedding-id order, documents without an embedding absent.  The
        label column is not touched (it belongs to the levels).  No topic, or more than 1,024, raises ValueError."""
        topics = _classify_topics(topics)
        _LOG.info(f"classifying every document by {len(topics)} topics")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        vecs = np.array(self._embed_chunked(topics), dtype=np.float32)
        _LOG.info("got embeddings for the topics!")
        assigned = self.embeddings_matrix.assign(vecs)   # one pass over the corpus: HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} x {len(topics)} cosine similarities")
        with self.db.transaction():
            doc_of = self.db.doc_ids_for_embeddings(None)
        res = _classified(assigned, doc_of, len(topics))
        _LOG.info(f"classified {len(res['doc_ids'])} documents")
        return res

    def cluster_documents(self, n_clusters: int, iterations: int = 10, seed: int = 0) -> Dict[str, Any]:
        """Unsupervised grouping: spherical k-means of the document embeddings into ``n_clusters`` clusters, every
        iteration on the device (svs_index_assign, then svs_index_label_sums) -- no embedding leaves HBM.  Returns
        {'doc_ids': int64 (m,), 'cluster': int32 (m,), 'score': float32 (m,), 'counts': int64 (n_clusters,),
        'centroids': float32 (n_clusters, D), 'iterations': int}: ``cluster[i]`` is the cluster of document
        ``doc_ids[i]`` and ``score[i]`` its similarity to the centroid it was assigned to; documents in embedding-id
        order, documents without an embedding absent.  The first centroids are ``n_clusters`` stored embeddings drawn
        with ``seed``; one seed gives one answer.  The label column is not touched (it belongs to the levels).  Fewer
        than one or more than 1,024 clusters, or more clusters than embeddings, raises ValueError."""
        _cluster_args(n_clusters, iterations)
        _LOG.info(f"clustering every document into {n_clusters} clusters")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        clustered = self.embeddings_matrix.cluster(int(n_clusters), int(iterations), int(seed))   # the whole loop: HIP
        _LOG.info(f"ran {clustered[5]} k-means iterations over {self.embeddings_matrix.index.shape[0]} embeddings")
        with self.db.transaction():
            doc_of = self.db.doc_ids_for_embeddings(None)
        res = _clustered(clustered, doc_of, int(n_clusters))
        _LOG.info(f"clustered {len(res['doc_ids'])} documents")
        return res

    def retrieve_diverse(self, query: str, n: int, fetch_n: Optional[int] = None, diversity: float = 0.5) -> List[Dict[str, Any]]:
        """``retrieve`` without the near-copies: the ``fetch_n`` best documents (default min(max(4 n, 32), 1024)) are
        re-ranked on the device by maximal marginal relevance (svs_index_search_diverse) -- greedily, by
        ``(1 - diversity) * score - diversity * (largest similarity to a document already picked)`` -- and ``n`` of
        them come back in PICK order, shaped like ``retrieve`` with a 'redundancy' key (that largest similarity when the
        document was picked; -inf for the first).  ``diversity=0`` is ``retrieve``.  ValueError for a diversity outside
        [0, 1], for ``n`` or ``fetch_n`` above 1024, and for ``fetch_n < n``."""
        fetch_k, lam = _diverse_args(n, fetch_n, diversity)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        picks = self.embeddings_matrix.search_diverse(query_vec, n, fetch_k, lam)   # HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        with self.db.transaction():
            res = _fetch_diverse(self.db, picks)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_combined(self, queries: List[str], n: int, mode: str = "any", weights=None) -> List[Dict[str, Any]]:
        """``retrieve`` against several query strings at once -- the rewordings of one question, the facets of a request,
        liked and disliked examples: the 1 .. 8 ``queries`` are embedded in one call and every document is ranked on the
        device (svs_index_search_combined) by its best score against any of them (``mode="any"``), by its worst (``"all"``:
        relevant to every one), or by the weighted sum of its scores (``"sum"``; negative ``weights`` push away).
        ``weights``: one finite number per query, or None for 1.  One pass over the corpus; results shaped like
        ``retrieve``, and ``retrieve_combined([q], n)`` is ``retrieve(q, n)``.  ValueError for no query or more than 8,
        an unknown mode, and bad weights."""
        queries, op, w = _combined_args(queries, mode, weights)
        _LOG.info(f"retrieving {n} documents with {len(queries)} query strings: {queries}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        query_vecs = np.array(self._embed(queries), dtype=np.float32)
        _LOG.info("got embeddings for the queries!")
        emb_ids = self.embeddings_matrix.search_combined(query_vecs, n, op, w)   # one pass + selection: HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} x {len(queries)} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_collapsed_combined(self, queries: List[str], n: int, mode: str = "any", weights=None) -> List[Dict[str, Any]]:
        """``retrieve_collapsed`` against several query strings at once: the n best PARENTS, where a parent's score
        against each query is its best child's and the per-query scores are combined as ``retrieve_combined`` combines a
        document's (``mode``, ``weights``: the same arguments and checks).  With ``mode="all"`` over two facets a parent
        whose one section answers the first facet and another section the second ranks high, which no single section
        does.  Each parent is represented by the child ``retrieve_combined`` would rank first; a document without a
        parent stands for itself.  Grouping and combination run on the device (svs_index_search_collapsed_combined)
        over the column ``retrieve_collapsed`` uses; results shaped like ``retrieve``, 'score' being the parent's."""
        queries, op, w = _combined_args(queries, mode, weights)
        _LOG.info(f"retrieving {n} documents with {len(queries)} query strings: {queries}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)

        def parents_from_store():
            with self.db.transaction():
                return self.db.embedding_parents()

        self.embeddings_matrix.ensure_column(PARENT_COLUMN, parents_from_store)
        query_vecs = np.array(self._embed(queries), dtype=np.float32)
        _LOG.info("got embeddings for the queries!")
        hits, _ = self.embeddings_matrix.search_collapsed_combined(query_vecs, n, PARENT_COLUMN, op, w, "single")   # one pass + grouping: HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} x {len(queries)} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, [(score, emb_id) for score, emb_id, _ in hits])
        _LOG.info(f"retrieved top {n} documents")
        return res

    def retrieve_similar(self, doc_id: int, n: int) -> List[Dict[str, Any]]:
        """"More like this": the n documents nearest to the STORED document ``doc_id``, itself excluded, shaped like
        ``retrieve`` ([{'score', 'doc'}]).  The reference can only loop ``np.dot(M, M[i])`` + ``get_top_k``
        (src/svs/kb.py:1623, src/svs/util.py:190-203); here the stored row is the query on the device
        (svs_index_neighbors).  An unknown doc raises KeyError, a doc without an embedding ValueError."""
        _LOG.info(f"retrieving {n} documents similar to document {doc_id}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        with self.db.transaction():
            emb = self.db.embedding_of_doc(doc_id)
        emb_ids = self.embeddings_matrix.neighbors([emb], n)[0]          # HIP
        _LOG.info(f"computed {self.embeddings_matrix.index.shape[0]} cosine similarities")
        with self.db.transaction():
            res = _fetch_list(self.db, emb_ids)
        _LOG.info(f"retrieved top {n} documents")
        return res

    def document_neighbors(self, n: int, doc_ids: Optional[List[int]] = None) -> List[Tuple[int, List[Tuple[float, int]]]]:
        """The kNN graph: [(doc_id, [(score, neighbour_doc_id), ...]), ...] for the listed docs, in the order given;
        ``doc_ids=None``: every doc that has an embedding, in embedding-id order.  Ids only, no records (feed
        them to ``fetch`` calls or an edge store as needed).  An unknown doc raises KeyError, a listed doc without
        an embedding ValueError."""
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        with self.db.transaction():
            pairs = self.db.docs_with_embeddings(None if doc_ids is None else list(doc_ids))
        _LOG.info(f"computing {n} neighbours of {len(pairs)} documents")
        per_doc = self.embeddings_matrix.neighbors([e for _, e in pairs], n)   # HIP
        with self.db.transaction():
            doc_of = self.db.doc_ids_for_embeddings(None if doc_ids is None else sorted({e for lst in per_doc for _, e in lst}))
        return [(d, [(s, doc_of[e]) for s, e in lst]) for (d, _), lst in zip(pairs, per_doc)]

    def document_top_pairwise_scores(self, n: int) -> List[Tuple[float, Dict[str, Any], Dict[str, Any]]]:
        """Reference src/svs/kb.py:1642-1671: the n most similar document pairs,
        [(score, doc_1, doc_2)].  M.M^T and the upper-triangle top-n run on the GPU
        (svs_index_top_pairs)."""
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        n_docs = self.embeddings_matrix.index.shape[0]
        _LOG.info(f"computing pairwise similarity over {n_docs} documents")
        pairs = self.embeddings_matrix.top_pairs(n)
        _LOG.info(f"computed {n_docs * n_docs} pairwise cosine similarities")
        with self.db.transaction():
            docs = self.db.fetch_docs_for_embeddings(sorted({e for _, a, b in pairs for e in (a, b)}))
        _LOG.info(f"retrieved top {n} document pairs")
        return [(score, docs[a], docs[b]) for score, a, b in pairs]

    def retrieve_many(self, queries: List[str], n: int) -> List[List[Dict[str, Any]]]:
        """Batched ``retrieve()``: the queries are embedded
        in chunks of 200 like bulk_add_docs, searched together (the corpus is read
        once per 16 queries instead of once per query) and each result list is
        fetched with one SQL statement.  Element i equals ``retrieve(queries[i], n)``."""
        _LOG.info(f"retrieving {n} documents for each of {len(queries)} query strings")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        vecs = self._embed_chunked(queries)
        if not vecs:
            return []
        per_query = self.embeddings_matrix.search_many(np.array(vecs, dtype=np.float32), n)
        with self.db.transaction():
            return _fetch_lists(self.db, per_query)

    def retrieve_many_within(self, queries: List[str], n: int, doc_id_lists: List[List[int]]) -> List[List[Dict[str, Any]]]:
        """``retrieve_within`` for many (query, doc list) pairs -- requests that each carry their own tenant, book or
        level: the queries are embedded in chunks of 200 like ``retrieve_many``, every list is scored and ranked in ONE
        native call (svs_index_search_segments) and fetched with one SQL statement.  Element i equals
        ``retrieve_within(queries[i], n, doc_id_lists[i])``.  An unknown doc id raises KeyError; docs without an
        embedding are skipped."""
        _LOG.info(f"retrieving {n} documents for each of {len(queries)} query strings, each within its own documents")
        if len(queries) != len(doc_id_lists):
            raise ValueError(f"{len(queries)} queries for {len(doc_id_lists)} document lists")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        with self.db.transaction():
            embs = [self.db.embeddings_for_docs(list(ids)) for ids in doc_id_lists]
        vecs = self._embed_chunked(queries)
        if not vecs:
            return []
        _LOG.info("got embeddings for the queries!")
        per_list = self.embeddings_matrix.search_within_many(np.array(vecs, dtype=np.float32), n, embs)   # HIP
        _LOG.info(f"computed {sum(len(e) for e in embs)} cosine similarities")
        with self.db.transaction():
            res = _fetch_lists(self.db, per_list)
        _LOG.info(f"retrieved top {n} documents for {len(queries)} queries")
        return res

    def retrieve_within_each(self, query: str, n: int, doc_id_lists: List[List[int]]) -> List[List[Dict[str, Any]]]:
        """The drill-down: ONE query against many doc lists (the children of each of the best sections), one
        embedding call and one native call (svs_index_search_segments).  Element g equals
        ``retrieve_within(query, n, doc_id_lists[g])``; nothing is merged across the lists.  An unknown doc id raises
        KeyError; docs without an embedding are skipped."""
        _LOG.info(f"retrieving {n} documents within each of {len(doc_id_lists)} document lists with query string: {query}")
        assert self.db is not None
        self.embeddings_matrix.get_sync(self.db)
        with self.db.transaction():
            embs = [self.db.embeddings_for_docs(list(ids)) for ids in doc_id_lists]
        if not embs:
            return []
        query_vec = np.array(self._embed([query])[0], dtype=np.float32)
        _LOG.info("got embedding for query!")
        per_list = self.embeddings_matrix.search_within_many(query_vec[None, :], n, embs, [0] * len(embs))   # HIP
        _LOG.info(f"computed {sum(len(e) for e in embs)} cosine similarities")
        with self.db.transaction():
            res = _fetch_lists(self.db, per_list)
        _LOG.info(f"retrieved top {n} documents for {len(embs)} lists")
        return res


class AsyncKB:
    """Async twin (reference src/svs/kb.py:925-1206): the matrix is fetched under
    the lock, ``superheavy`` runs on an executor thread OUTSIDE the lock
    (:1184-1190), so concurrent retrieve() calls search the same handle
    concurrently -- the C ABI is re-entrant for exactly this."""

    def __init__(self, local_path: str, embedding_func: Optional[EmbeddingFunc] = None,
                 device: int = 0, index_factory: Callable[..., Any] = DeviceIndex, dtype: str = "f32"):
        if embedding_func is None:
            raise RuntimeError("No embedding function. You must pass the embedding function you want to use.")
        self.embedding_func = embedding_func
        self._path = local_path
        self.db: Optional[_Store] = None
        self._lock: Optional[asyncio.Lock] = None
        self.embeddings_matrix = _device_matrix(device, index_factory, dtype)

    def _get_lock(self) -> asyncio.Lock:
        if self._lock is None:
            self._lock = asyncio.Lock()
        return self._lock

    async def _ensure_db(self) -> _Store:
        if self.db is None:
            loop = asyncio.get_running_loop()
            self.db = await loop.run_in_executor(None, lambda: _Store(self._path))
        return self.db

    async def _embed(self, texts: List[str]) -> List[List[float]]:
        vectors = await self.embedding_func(texts)
        check_magnitude(vectors)
        return vectors

    async def _embed_chunked(self, texts: List[str]) -> List[List[float]]:
        return [vec for chunk in _chunks(texts) for vec in await self._embed(chunk)]

    # -- the frame of every retrieval: SQL and the reference to the index under the lock, the embedding and the search
    # -- outside it, the documents under the lock again (reference src/svs/kb.py:1171-1206)
    @staticmethod
    async def _in_transaction(db: _Store, work: Callable[[_Store], Any]) -> Any:
        """``work(db)`` inside one transaction, on an executor thread; the caller holds the lock."""
        def run():
            with db.transaction():
                return work(db)

        return await asyncio.get_running_loop().run_in_executor(None, run)

    @asynccontextmanager
    async def _held(self, sql: Optional[Callable[[_Store], Any]] = None, single: bool = False):
        """Entry, under the lock: the store, the loaded matrix, ``sql(db)`` (if given: the doc id -> embedding id
        queries, in a transaction on an executor thread; what it raises leaves before any reference is taken), then
        ``hold()`` -- ``hold_search()`` for ``single`` -- so that a later invalidate() cannot affect this search.
        Yields (held, what ``sql`` returned) with the lock FREE: the body embeds and searches while other tasks use
        the KB.  Releases the index however the body ends: a return, an exception, a cancellation."""
        async with self._get_lock():
            db = await self._ensure_db()
            await self.embeddings_matrix.get(db)
            found = await self._in_transaction(db, sql) if sql is not None else None
            held = self.embeddings_matrix.hold_search() if single else self.embeddings_matrix.hold()
        try:
            yield held, found
        finally:
            held[0].release()

    async def _search(self, held: tuple, op, single: bool = False):
        """One mapped search of svs_amd.matrix on an executor thread, against the reference ``_held`` yielded."""
        return await asyncio.get_running_loop().run_in_executor(None, lambda: self.embeddings_matrix.run_mapped(op, held, single))

    async def _fetch(self, work: Callable[[_Store], Any]) -> Any:
        """``heavy()``: ``work(db)`` under the lock, inside one transaction, on an executor thread."""
        async with self._get_lock():
            return await self._in_transaction(await self._ensure_db(), work)

    async def load(self) -> None:
        async with self._get_lock():
            db = await self._ensure_db()
            await self.embeddings_matrix.get(db)

    async def close(self) -> None:
        async with self._get_lock():
            if self.db is not None:
                self.db.close()
                self.db = None
            self.embeddings_matrix.invalidate()

    async def count(self) -> int:
        async with self._get_lock():
            db = await self._ensure_db()
            with db.transaction():
                return db.count_docs()

    @asynccontextmanager
    async def bulk_add_docs(self):
        async with self._get_lock():
            db = await self._ensure_db()
            pending: List[Tuple[int, str, int, Optional[int]]] = []
            live = True
            db.conn.execute("BEGIN")
            try:
                async def add_doc(text: str, parent_id: Optional[int] = None,
                                  meta: Optional[Dict[str, Any]] = None, no_embedding: bool = False) -> int:
                    assert live, "You may not call this function outside of the context manager!"
                    doc_id, level = db.add_doc_at(text, parent_id, meta)
                    if not no_embedding:
                        pending.append((doc_id, text, level, parent_id))
                    return doc_id
                try:
                    yield add_doc
                finally:
                    live = False
                new_ids: List[int] = []
                new_vecs: List[List[float]] = []
                new_labels: List[int] = []     # level + 1 of every new embedding's doc (retrieve_at_level)
                new_parents: List[Optional[int]] = []   # its parent id (retrieve_under)
                for c0 in range(0, len(pending), BULK_EMBEDDING_CHUNK_SIZE):
                    chunk = pending[c0:c0 + BULK_EMBEDDING_CHUNK_SIZE]
                    vectors = await self._embed([c[1] for c in chunk])
                    for (doc_id, _, level, parent_id), vec in zip(chunk, vectors):
                        new_ids.append(db.set_doc_embedding(doc_id, embedding_to_bytes(vec)))
                        new_vecs.append(vec)
                        new_labels.append(level + 1)
                        new_parents.append(parent_id)
            except BaseException:
                db.conn.execute("ROLLBACK")
                self.embeddings_matrix.invalidate()
                raise
            else:
                db.conn.execute("COMMIT")
            if new_ids:   # extend the HBM copy in place (reference: invalidate(), kb.py:1062)
                loop = asyncio.get_running_loop()
                await loop.run_in_executor(None, lambda: self.embeddings_matrix.append(
                    np.array(new_vecs, dtype=np.float32), new_ids, labels=new_labels,
                    columns={PARENT_COLUMN: _parent_column(new_parents)}))

    @asynccontextmanager
    async def bulk_del_docs(self):
        async with self._get_lock():
            db = await self._ensure_db()
            live = True
            gone: List[int] = []
            db.conn.execute("BEGIN")
            try:
                async def del_doc(doc_id: int) -> None:
                    assert live, "You may not call this function outside of the context manager!"
                    emb_id = db.del_doc(doc_id)
                    if emb_id is not None:
                        gone.append(emb_id)
                try:
                    yield del_doc
                finally:
                    live = False
            except BaseException:
                db.conn.execute("ROLLBACK")
                self.embeddings_matrix.invalidate()
                raise
            else:
                db.conn.execute("COMMIT")
            if gone:      # tombstone in HBM (reference: invalidate(), kb.py:1086)
                self.embeddings_matrix.remove(gone)

    async def retrieve(self, query: str, n: int) -> List[Dict[str, Any]]:
        """Reference src/svs/kb.py:1171-1206."""
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        async with self._held(single=True) as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            # tasks whose searches are in flight together share corpus passes (svs_amd/coalesce.py)
            emb_ids = await self._search(held, single_op(query_vec, n), single=True)
            _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
        res = await self._fetch(lambda db: [{"score": s, "doc": db.fetch_doc_for_embedding(e)} for s, e in emb_ids])
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_within(self, query: str, n: int, doc_ids: List[int]) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_within``, structured as ``retrieve``: the SQL and the reference to the
        matrix under the lock, the filtered search on an executor thread outside it, the docs under the lock."""
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        ids = list(doc_ids)
        async with self._held(lambda db: db.embeddings_for_docs(ids)) as (held, emb):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            emb_ids = await self._search(held, within_op(query_vec, n, emb))
            _LOG.info(f"computed {len(emb)} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_above(self, query: str, min_score: float, n: int) -> Tuple[List[Dict[str, Any]], int]:
        """Async twin of ``KB.retrieve_above``, structured as ``retrieve``: the reference to the matrix under the
        lock, the threshold search on an executor thread outside it, the docs under the lock."""
        if min_score != min_score:
            raise ValueError("min_score is NaN")
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        async with self._held() as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            emb_ids, total = await self._search(held, above_op(query_vec, float(min_score), n))
            _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res, total

    async def retrieve_at_level(self, query: str, n: int, levels) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_at_level``, structured as ``retrieve``: the label column is installed (when this
        index generation has none yet) and the reference to the matrix is taken under the lock, the labelled search
        runs on an executor thread outside it, the docs are fetched under the lock."""
        labels = _level_labels(levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        async with self._held(lambda db: self.embeddings_matrix.ensure_labels(db.embedding_levels)) as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            emb_ids, matched = await self._search(held, labeled_op(query_vec, n, labels))
            _LOG.info(f"computed {matched} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_under(self, query: str, n: int, parent_ids, levels=None) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_under``, structured as ``retrieve_at_level``: the columns are installed (when
        this index generation lacks them) and the reference to the matrix is taken under the lock, the predicate search
        runs on an executor thread outside it, the docs are fetched under the lock."""
        where = _under_where(parent_ids, levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")

        def install(db):
            self.embeddings_matrix.ensure_column(PARENT_COLUMN, db.embedding_parents)
            if levels is not None:
                self.embeddings_matrix.ensure_labels(db.embedding_levels)

        async with self._held(install) as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            emb_ids, matched = await self._search(held, where_op(query_vec, n, where))
            _LOG.info(f"computed {matched} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_collapsed(self, query: str, n: int, levels=None) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_collapsed``, structured as ``retrieve_under``: the columns are installed (when
        this index generation lacks them) and the reference to the matrix is taken under the lock, the collapsed search
        runs on an executor thread outside it, the docs are fetched under the lock."""
        labels = None if levels is None else _level_labels(levels)
        _LOG.info(f"retrieving {n} documents with query string: {query}")

        def install(db):
            self.embeddings_matrix.ensure_column(PARENT_COLUMN, db.embedding_parents)
            if labels is not None:
                self.embeddings_matrix.ensure_labels(db.embedding_levels)

        async with self._held(install) as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            if labels is None:
                hits, _ = await self._search(held, collapsed_op(query_vec, n, PARENT_COLUMN, "single"))
                _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
            else:
                hits, _, matched = await self._search(held, collapsed_where_op(query_vec, n, [(0, "in", labels)], PARENT_COLUMN, "single"))
                _LOG.info(f"computed {matched} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, [(score, emb_id) for score, emb_id, _ in hits]))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_by_level(self, query: str, min_score: Optional[float] = None, levels=None) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_by_level``, structured as ``retrieve``: the label column is installed (when this
        index generation has none yet), the levels of the store are read (``levels=None``) and the reference to the
        matrix is taken under the lock, the breakdown runs on an executor thread outside it, the docs are fetched
        under the lock."""
        cut = _by_level_cut(min_score)
        given = None if levels is None else _level_labels(levels)
        _LOG.info(f"retrieving the best document of {'every level' if given is None else f'{len(given)} levels'} with query string: {query}")

        def prepare(db):
            self.embeddings_matrix.ensure_labels(db.embedding_levels)
            return given if given is not None else _level_labels(db.embedded_levels())

        async with self._held(prepare) as (held, labels):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            groups = await self._search(held, by_label_op(query_vec, labels, cut)) if labels else []
            _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
        res = await self._fetch(lambda db: _fetch_by_level(db, groups))
        _LOG.info(f"retrieved the best documents of {len(res)} levels")
        return res

    async def classify_documents(self, topics: List[str]) -> Dict[str, np.ndarray]:
        """Async twin of ``KB.classify_documents``, structured as ``retrieve_many``: the reference to the matrix under
        the lock, the embedding and the one assignment call on an executor thread outside it, the doc ids under the
        lock."""
        topics = _classify_topics(topics)
        _LOG.info(f"classifying every document by {len(topics)} topics")
        async with self._held() as (held, _):
            vecs = np.array(await self._embed_chunked(topics), dtype=np.float32)
            _LOG.info("got embeddings for the topics!")
            assigned = await self._search(held, assign_op(vecs))
            _LOG.info(f"computed {held[0].shape[0]} x {len(topics)} cosine similarities")
        doc_of = await self._fetch(lambda db: db.doc_ids_for_embeddings(None))
        res = _classified(assigned, doc_of, len(topics))
        _LOG.info(f"classified {len(res['doc_ids'])} documents")
        return res

    async def cluster_documents(self, n_clusters: int, iterations: int = 10, seed: int = 0) -> Dict[str, Any]:
        """Async twin of ``KB.cluster_documents``, structured as ``classify_documents``: the reference to the matrix
        under the lock, the whole k-means loop as ONE mapped call on an executor thread outside it, the doc ids under
        the lock."""
        _cluster_args(n_clusters, iterations)
        _LOG.info(f"clustering every document into {n_clusters} clusters")
        async with self._held() as (held, _):
            clustered = await self._search(held, cluster_op(int(n_clusters), int(iterations), int(seed)))
            _LOG.info(f"ran {clustered[5]} k-means iterations over {held[0].shape[0]} embeddings")
        doc_of = await self._fetch(lambda db: db.doc_ids_for_embeddings(None))
        res = _clustered(clustered, doc_of, int(n_clusters))
        _LOG.info(f"clustered {len(res['doc_ids'])} documents")
        return res

    async def retrieve_diverse(self, query: str, n: int, fetch_n: Optional[int] = None,
                               diversity: float = 0.5) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_diverse``, structured as ``retrieve``: the reference to the matrix under the
        lock, the diverse search on an executor thread outside it, the docs under the lock."""
        fetch_k, lam = _diverse_args(n, fetch_n, diversity)
        _LOG.info(f"retrieving {n} documents with query string: {query}")
        async with self._held() as (held, _):
            query_vec = np.array((await self._embed([query]))[0], dtype=np.float32)
            _LOG.info("got embedding for query!")
            picks = await self._search(held, diverse_op(query_vec, n, fetch_k, lam))
            _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
        res = await self._fetch(lambda db: _fetch_diverse(db, picks))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_combined(self, queries: List[str], n: int, mode: str = "any", weights=None) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_combined``, structured as ``retrieve``: the reference to the matrix under the
        lock, the one embedding call and the combined search on an executor thread outside it, the docs under the lock."""
        queries, op, w = _combined_args(queries, mode, weights)
        _LOG.info(f"retrieving {n} documents with {len(queries)} query strings: {queries}")
        async with self._held() as (held, _):
            query_vecs = np.array(await self._embed(queries), dtype=np.float32)
            _LOG.info("got embeddings for the queries!")
            emb_ids = await self._search(held, combined_op(query_vecs, n, op, w))
            _LOG.info(f"computed {held[0].shape[0]} x {len(queries)} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_collapsed_combined(self, queries: List[str], n: int, mode: str = "any", weights=None) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_collapsed_combined``, structured as ``retrieve_collapsed``: the parent column is
        installed and the reference to the matrix is taken under the lock, the one embedding call and the search run
        outside it, the docs are fetched under the lock."""
        queries, op, w = _combined_args(queries, mode, weights)
        _LOG.info(f"retrieving {n} documents with {len(queries)} query strings: {queries}")
        async with self._held(lambda db: self.embeddings_matrix.ensure_column(PARENT_COLUMN, db.embedding_parents)) as (held, _):
            query_vecs = np.array(await self._embed(queries), dtype=np.float32)
            _LOG.info("got embeddings for the queries!")
            hits, _ = await self._search(held, collapsed_combined_op(query_vecs, n, PARENT_COLUMN, op, w, "single"))
            _LOG.info(f"computed {held[0].shape[0]} x {len(queries)} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, [(score, emb_id) for score, emb_id, _ in hits]))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def retrieve_many(self, queries: List[str], n: int) -> List[List[Dict[str, Any]]]:
        """Async twin of ``KB.retrieve_many``.  Same structure as
        ``retrieve`` (reference src/svs/kb.py:1171-1206): the matrix is fetched under the lock, the
        batched search runs on an executor thread OUTSIDE it on a held reference, and every result
        list is fetched with one ``IN (...)`` statement.  Element i equals ``retrieve(queries[i], n)``."""
        _LOG.info(f"retrieving {n} documents for each of {len(queries)} query strings")
        async with self._held() as (held, _):
            vecs = await self._embed_chunked(queries)
            if not vecs:
                return []
            _LOG.info("got embeddings for the queries!")
            per_query = await self._search(held, batch_op(np.array(vecs, dtype=np.float32), n))
            _LOG.info(f"computed {held[0].shape[0]} x {len(vecs)} cosine similarities")
        res = await self._fetch(lambda db: _fetch_lists(db, per_query))
        _LOG.info(f"retrieved top {n} documents for {len(queries)} queries")
        return res

    async def _retrieve_segments(self, texts: List[str], n: int, doc_id_lists: List[List[int]], one_query: bool,
                                 embedded: str, done: str) -> List[List[Dict[str, Any]]]:
        """The body of ``retrieve_many_within`` (one query per list) and ``retrieve_within_each`` (``one_query``),
        structured as ``retrieve_within``: the SQL and the reference to the matrix under the lock, the segmented
        search on an executor thread outside it, the docs under the lock."""
        lists = [list(ids) for ids in doc_id_lists]
        async with self._held(lambda db: [db.embeddings_for_docs(ids) for ids in lists]) as (held, embs):
            if not embs:
                return []
            vecs = await self._embed_chunked(texts)
            _LOG.info(embedded)
            seg_query = [0] * len(embs) if one_query else None
            per_list = await self._search(held, segments_op(np.array(vecs, dtype=np.float32), n, embs, seg_query))
            _LOG.info(f"computed {sum(len(e) for e in embs)} cosine similarities")
        res = await self._fetch(lambda db: _fetch_lists(db, per_list))
        _LOG.info(done)
        return res

    async def retrieve_many_within(self, queries: List[str], n: int, doc_id_lists: List[List[int]]) -> List[List[Dict[str, Any]]]:
        """Async twin of ``KB.retrieve_many_within``: element i equals ``retrieve_within(queries[i], n, doc_id_lists[i])``."""
        _LOG.info(f"retrieving {n} documents for each of {len(queries)} query strings, each within its own documents")
        if len(queries) != len(doc_id_lists):
            raise ValueError(f"{len(queries)} queries for {len(doc_id_lists)} document lists")
        return await self._retrieve_segments(list(queries), n, doc_id_lists, False, "got embeddings for the queries!",
                                             f"retrieved top {n} documents for {len(queries)} queries")

    async def retrieve_within_each(self, query: str, n: int, doc_id_lists: List[List[int]]) -> List[List[Dict[str, Any]]]:
        """Async twin of ``KB.retrieve_within_each``: element g equals ``retrieve_within(query, n, doc_id_lists[g])``."""
        _LOG.info(f"retrieving {n} documents within each of {len(doc_id_lists)} document lists with query string: {query}")
        return await self._retrieve_segments([query], n, doc_id_lists, True, "got embedding for query!",
                                             f"retrieved top {n} documents for {len(doc_id_lists)} lists")

    async def retrieve_similar(self, doc_id: int, n: int) -> List[Dict[str, Any]]:
        """Async twin of ``KB.retrieve_similar``, structured as ``retrieve``: the SQL and the reference to the matrix
        under the lock, svs_index_neighbors on an executor thread outside it, the docs under the lock."""
        _LOG.info(f"retrieving {n} documents similar to document {doc_id}")
        async with self._held(lambda db: db.embedding_of_doc(doc_id)) as (held, emb):
            emb_ids = (await self._search(held, neighbors_op([emb], n)))[0]
            _LOG.info(f"computed {held[0].shape[0]} cosine similarities")
        res = await self._fetch(lambda db: _fetch_list(db, emb_ids))
        _LOG.info(f"retrieved top {n} documents")
        return res

    async def document_neighbors(self, n: int, doc_ids: Optional[List[int]] = None) -> List[Tuple[int, List[Tuple[float, int]]]]:
        """Async twin of ``KB.document_neighbors``: ids only; the native call on an executor thread outside the lock."""
        ids = None if doc_ids is None else list(doc_ids)
        async with self._held(lambda db: db.docs_with_embeddings(ids)) as (held, pairs):
            _LOG.info(f"computing {n} neighbours of {len(pairs)} documents")
            per_doc = await self._search(held, neighbors_op([e for _, e in pairs], n))
        doc_of = await self._fetch(lambda db: db.doc_ids_for_embeddings(
            None if ids is None else sorted({e for lst in per_doc for _, e in lst})))
        return [(d, [(s, doc_of[e]) for s, e in lst]) for (d, _), lst in zip(pairs, per_doc)]

    async def document_top_pairwise_scores(self, n: int) -> List[Tuple[float, Dict[str, Any], Dict[str, Any]]]:
        """Reference src/svs/kb.py:1208-1243 (async twin of :1642-1671): the n most similar document
        pairs, [(score, doc_1, doc_2)].  ``superheavy`` -- there ``np.dot(M, M.T)`` + ``get_top_pairs``
        (src/svs/kb.py:1219, src/svs/util.py:206-233) -- is svs_index_top_pairs on an executor
        thread, outside the lock, on a held reference."""
        async with self._held() as (held, _):
            n_docs = held[0].shape[0]
            _LOG.info(f"computing pairwise similarity over {n_docs} documents")
            pairs = await self._search(held, pairs_op(n))
            _LOG.info(f"computed {n_docs * n_docs} pairwise cosine similarities")
        docs = await self._fetch(lambda db: db.fetch_docs_for_embeddings(sorted({e for _, a, b in pairs for e in (a, b)})))
        _LOG.info(f"retrieved top {n} document pairs")
        return [(score, docs[a], docs[b]) for score, a, b in pairs]

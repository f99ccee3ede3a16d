"""CPU: the KB mirror reclaims tombstoned rows by compacting the loaded index in place instead of rebuilding it
from SQLite (svs_amd/matrix.py: DeviceEmbeddingsMatrix.remove, _Lookup.stale, search_mapped).  The index here is a
test double whose arithmetic is the numpy oracle; what is under test is the host logic: which branch ``remove``
takes, the renumbered lookup, and a search that was between ``hold()`` and its native call while the rows moved."""
import asyncio
import threading

import numpy as np
import pytest

import above_model
from fake_backend import OracleIndex
from oracle import svs_oracle as oracle

import svs_amd
from svs_amd import matrix as mx


class CompactingOracleIndex(OracleIndex):
    """OracleIndex with ``compact()`` (and ``search_within``, ``search_segments``, ``search_above``).  Like the library, a compaction and a search exclude
    each other.  ``gate = (entered, go)`` parks the NEXT native search call of any owner: it sets ``entered`` and
    waits for ``go`` before it computes anything, i.e. it sits between ``hold()`` and the native call."""

    gate = None
    compactions = 0
    _geo = threading.RLock()

    def share(self):
        self._check()
        return CompactingOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def compact(self):
        self._check()
        with CompactingOracleIndex._geo:
            keep = np.flatnonzero(~self._st[1])
            self._st[0] = np.ascontiguousarray(self._st[0][keep])
            self._st[1] = np.zeros(len(keep), dtype=bool)
            CompactingOracleIndex.compactions += 1
            return keep + self.row_offset

    @staticmethod
    def _park():
        gate, CompactingOracleIndex.gate = CompactingOracleIndex.gate, None
        if gate is not None:
            gate[0].set()
            assert gate[1].wait(30)

    def search(self, q, n):
        self._park()
        with CompactingOracleIndex._geo:
            return super().search(q, n)

    def search_batch(self, queries, n):
        self._park()
        with CompactingOracleIndex._geo:
            return super().search_batch(queries, n)

    def top_pairs(self, n):
        self._park()
        with CompactingOracleIndex._geo:
            return super().top_pairs(n)

    def search_within(self, q, n, rows):
        self._park()
        with CompactingOracleIndex._geo:
            self._check()
            local = np.unique(np.asarray(rows, dtype=np.int64)) - self.row_offset
            if len(local) and (local[0] < 0 or local[-1] >= self.n):
                raise ValueError("row out of range")
            s = local[~self._st[1][local]]
            return [(sc, int(s[p]) + self.row_offset) for sc, p in oracle.cpu_search(self._m[s], np.asarray(q, dtype=np.float32), n)]

    def search_segments(self, queries, n, row_lists, seg_query=None):
        self._park()
        with CompactingOracleIndex._geo:
            q = np.ascontiguousarray(queries, dtype=np.float32)
            row_lists = list(row_lists)
            if seg_query is None:
                if len(row_lists) != len(q):
                    raise ValueError("one row list per query")
                seg_query = range(len(q))
            out = []
            for rows, j in zip(row_lists, seg_query):
                res = self.search_within(q[j], n, rows)
                out.append((np.array([a for a, _ in res], dtype=np.float32), np.array([b for _, b in res], dtype=np.int64)))
            return out

    def search_above(self, q, min_score, limit):
        self._park()
        with CompactingOracleIndex._geo:
            self._check()
            q = np.asarray(q, dtype=np.float32)
            rows, sc, total = above_model.above(oracle.cpu_scores(self._m, q), self._st[1], np.float32(min_score), limit)
            return list(zip(sc.astype(np.float64).tolist(), (rows + self.row_offset).tolist())), total


N_DOCS, DIM = 240, 24


def _table():
    rng = np.random.default_rng(31)
    vecs = rng.standard_normal((N_DOCS + 40, DIM))
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    return {f"doc {i}": [float(x) for x in vecs[i]] for i in range(len(vecs))}


TABLE = _table()


async def _ef(texts):
    return [TABLE[t] for t in texts]


def _loaded_kb(path, index_factory, **matrix_kw):
    """A KB of N_DOCS docs (doc id == i + 1), loaded, whose SQLite matrix builder counts its calls."""
    kb = svs_amd.KB(path, _ef, index_factory=index_factory)
    for k, v in matrix_kw.items():
        setattr(kb.embeddings_matrix, k, v)
    built = []
    inner = kb.embeddings_matrix._builder

    def counting(db):
        built.append(1)
        return inner(db)

    kb.embeddings_matrix._builder = counting
    if len(kb) == 0:
        with kb.bulk_add_docs() as add_doc:
            for i in range(N_DOCS):
                add_doc(f"doc {i}")
    kb.load()
    return kb, built


def _delete(kb, docs):
    with kb.bulk_del_docs() as del_doc:
        for i in docs:
            del_doc(i + 1)


def _ids(res):
    return [(d["doc"]["id"], d["score"]) for d in res]


def _same_answers(kb, fresh, gone):
    for q in ("doc 3", "doc 70", "doc 239", "doc 250"):
        assert _ids(kb.retrieve(q, 9)) == _ids(fresh.retrieve(q, 9)), q
    alive = [i + 1 for i in range(0, N_DOCS, 3) if i not in gone]
    assert _ids(kb.retrieve_within("doc 5", 7, alive)) == _ids(fresh.retrieve_within("doc 5", 7, alive))
    qs = ["doc 1", "doc 100", "doc 260"]
    assert [_ids(r) for r in kb.retrieve_many(qs, 6)] == [_ids(r) for r in fresh.retrieve_many(qs, 6)]
    assert [(s, a["id"], b["id"]) for s, a, b in kb.document_top_pairwise_scores(15)] == \
           [(s, a["id"], b["id"]) for s, a, b in fresh.document_top_pairwise_scores(15)]


def test_deletes_past_the_threshold_compact_in_place(tmp_path):
    path = str(tmp_path / "c.sqlite")
    kb, built = _loaded_kb(path, CompactingOracleIndex)
    first, before = kb.embeddings_matrix.index, CompactingOracleIndex.compactions
    assert len(built) == 1
    gone = {3, 50, 200}
    _delete(kb, sorted(gone))                                # tombstones only
    assert CompactingOracleIndex.compactions == before and first.shape[0] == N_DOCS
    more = list(range(60, 130)) + [0, 239]                   # 75 of 240 dead: past COMPACT_AT
    _delete(kb, more)
    gone |= set(more)
    assert CompactingOracleIndex.compactions == before + 1
    assert kb.embeddings_matrix.index is first and len(built) == 1
    assert first.shape[0] == N_DOCS - 75 and len(kb.embeddings_matrix.emb_id_lookup) == N_DOCS - 75
    fresh = svs_amd.KB(path, _ef, index_factory=CompactingOracleIndex)
    _same_answers(kb, fresh, gone)
    assert len(kb.retrieve("doc 1", 1000)) == N_DOCS - 75
    # the edited copy goes on working: append, tombstone, and a second compaction of the same object
    with kb.bulk_add_docs() as add_doc:
        for i in range(N_DOCS, N_DOCS + 20):
            add_doc(f"doc {i}")
    _delete(kb, (10, 245))
    assert kb.embeddings_matrix.index is first and CompactingOracleIndex.compactions == before + 1
    _delete(kb, range(130, 180))
    gone |= {10, 245} | set(range(130, 180))
    assert kb.embeddings_matrix.index is first and CompactingOracleIndex.compactions == before + 2 and len(built) == 1
    fresh.close()
    fresh = svs_amd.KB(path, _ef, index_factory=CompactingOracleIndex)
    _same_answers(kb, fresh, gone)
    kb.close(); fresh.close()
    assert OracleIndex.live == 0


@pytest.mark.parametrize("what", ["search", "search_within", "search_many", "top_pairs", "search_within_many", "search_above"])
def test_search_parked_across_a_compaction_retries(tmp_path, what):
    """The search holds (index, old lookup) and is parked in front of its native call; the compaction renumbers the
    rows; the search then runs on the new numbering, finds its lookup stale and repeats on a fresh hold."""
    path = str(tmp_path / "r.sqlite")
    kb, built = _loaded_kb(path, CompactingOracleIndex)
    cache = kb.embeddings_matrix
    first, old_lookup = cache.index, cache._lookup
    q = np.array(TABLE["doc 200"], dtype=np.float32)
    keep_ids = [int(e) for e in cache.emb_id_lookup[150:240:2]]
    def calls_on(c):
        return {"search": lambda: c.search(q, 8), "search_within": lambda: c.search_within(q, 8, keep_ids),
                "search_many": lambda: c.search_many(np.stack([q, -q]), 8), "top_pairs": lambda: c.top_pairs(8),
                "search_within_many": lambda: c.search_within_many(np.stack([q, -q]), 8, [keep_ids, keep_ids[::3]]),
                "search_above": lambda: c.search_above(q, 0.1, 8)}

    calls = calls_on(cache)
    entered, go = threading.Event(), threading.Event()
    CompactingOracleIndex.gate = (entered, go)
    out = {}

    def worker():
        try:
            out["res"] = calls[what]()
        except BaseException as e:  # noqa: BLE001
            out["err"] = e

    t = threading.Thread(target=worker)
    t.start()
    try:
        assert entered.wait(30)
        before = CompactingOracleIndex.compactions
        _delete(kb, range(20, 100))                          # 80 of 240: compacts while the search is parked
        assert CompactingOracleIndex.compactions == before + 1 and cache.index is first
        assert old_lookup.stale and cache._lookup is not old_lookup and not cache._lookup.stale
        assert len(old_lookup.arr) == N_DOCS                 # the old table is left as it was
    finally:
        go.set()
        t.join(60)
    assert "err" not in out, out.get("err")
    assert out["res"] == calls[what]()                       # the same call on the settled cache
    fresh = svs_amd.KB(path, _ef, index_factory=CompactingOracleIndex)
    fresh.load()
    want = calls_on(fresh.embeddings_matrix)[what]()
    assert out["res"] == want and len(built) == 1
    kb.close(); fresh.close()
    assert OracleIndex.live == 0


def test_async_kb_compacts_in_place(tmp_path):
    path = str(tmp_path / "a.sqlite")

    async def run():
        akb = svs_amd.AsyncKB(path, _ef, index_factory=CompactingOracleIndex)
        async with akb.bulk_add_docs() as add_doc:
            for i in range(N_DOCS):
                await add_doc(f"doc {i}")
        await akb.load()
        first, before = akb.embeddings_matrix.index, CompactingOracleIndex.compactions
        async with akb.bulk_del_docs() as del_doc:
            for i in range(100, 170):
                await del_doc(i + 1)
        assert akb.embeddings_matrix.index is first and CompactingOracleIndex.compactions == before + 1
        fresh = svs_amd.AsyncKB(path, _ef, index_factory=CompactingOracleIndex)
        docs = [i + 1 for i in range(0, 90, 2)]
        for kb_call in (lambda k: k.retrieve("doc 7", 9), lambda k: k.retrieve_within("doc 7", 5, docs),
                        lambda k: k.retrieve_many(["doc 8", "doc 230"], 4), lambda k: k.document_top_pairwise_scores(6)):
            a, b = await kb_call(akb), await kb_call(fresh)
            assert repr(a) == repr(b)
        await akb.close(); await fresh.close()

    asyncio.run(run())
    assert OracleIndex.live == 0


def test_index_without_compact_still_rebuilds(tmp_path):
    kb, built = _loaded_kb(str(tmp_path / "p.sqlite"), OracleIndex)
    first = kb.embeddings_matrix.index
    _delete(kb, range(60, 130))
    assert kb.embeddings_matrix.index is None and len(built) == 1
    assert len(kb.retrieve("doc 1", 1000)) == N_DOCS - 70
    assert kb.embeddings_matrix.index is not first and len(built) == 2
    kb.close()
    assert OracleIndex.live == 0


@pytest.mark.parametrize("setting", ["view", "keep_host"])
def test_view_and_host_copy_still_rebuild(tmp_path, setting):
    kw = {"_view": True} if setting == "view" else {"_keep_host": True}
    kb, built = _loaded_kb(str(tmp_path / "v.sqlite"), CompactingOracleIndex, **kw)
    before = CompactingOracleIndex.compactions
    first = kb.embeddings_matrix.index
    _delete(kb, range(60, 130))
    assert kb.embeddings_matrix.index is None and CompactingOracleIndex.compactions == before
    kb.load()
    assert kb.embeddings_matrix.index is not first and len(built) == 2 and kb.embeddings_matrix.index.shape[0] == N_DOCS - 70
    kb.close()
    assert OracleIndex.live == 0


def test_failed_compaction_drops_the_cache(tmp_path):
    """A device error half way leaves the rows in no defined order: the cache invalidates and rebuilds."""
    class Failing(CompactingOracleIndex):
        def share(self):
            self._check()
            return Failing(None, self.device, self.row_offset, _shared=self._st)

        def compact(self):
            raise RuntimeError("device error")

    kb, built = _loaded_kb(str(tmp_path / "f.sqlite"), Failing)
    old_lookup = kb.embeddings_matrix._lookup
    _delete(kb, range(60, 130))
    assert kb.embeddings_matrix.index is None and old_lookup.stale
    assert len(kb.retrieve("doc 1", 1000)) == N_DOCS - 70 and len(built) == 2
    kb.close()
    assert OracleIndex.live == 0


def test_search_mapped_keeps_errors_of_a_current_lookup():
    """An exception of the native call is swallowed only when the lookup went stale (it may come from rows of the
    old numbering); otherwise it is the caller's."""
    lk = mx._Lookup(np.array([5, 6, 7]))

    def boom(idx, lookup):
        raise ValueError("bad query")

    with pytest.raises(ValueError):
        mx.search_mapped(lambda: pytest.fail("no retry expected"), (object(), lk), boom, lambda r, a: r)

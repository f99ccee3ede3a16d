"""CPU: neighbours of stored rows above the kernel -- doc id -> emb id -> row and back in ``KB.retrieve_similar`` /
``KB.document_neighbors`` and their async twins, ``DeviceEmbeddingsMatrix.neighbors``, and a call that sits between
``hold()`` and its native call while a compaction renumbers the rows.  The index is a numpy double of DeviceIndex
(``neighbors`` = ``search_batch`` at n + 1 with the source row removed); svs_index_neighbors itself is checked on the
GPU (tests/test_neighbors_gpu.py)."""
import asyncio
import threading

import numpy as np
import pytest

from fake_backend import OracleIndex
from test_compact_host import CompactingOracleIndex

import svs_amd
from svs_amd import _native


class NeighborsOracleIndex(CompactingOracleIndex):
    """CompactingOracleIndex that also answers ``neighbors``: per row, the oracle search of the stored row at n + 1,
    the row itself removed (or, if it is not among them, the last entry dropped)."""

    calls = 0

    def share(self):
        self._check()
        return NeighborsOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def neighbors(self, rows, n):
        self._park()
        with CompactingOracleIndex._geo:
            self._check()
            NeighborsOracleIndex.calls += 1
            r = np.asarray(rows, dtype=np.int64).reshape(-1)
            local = r - self.row_offset
            if len(local) and (local.min() < 0 or local.max() >= self.n):
                raise ValueError("row out of range")
            if self._st[1][local].any():
                raise ValueError("row is tombstoned")
            count = min(max(n, 0), max(int((~self._st[1]).sum()) - 1, 0))
            s, g = OracleIndex.search_batch(self, self._m[local], count + 1) if len(r) else \
                (np.empty((0, count + 1), np.float32), np.empty((0, count + 1), np.int64))
            out_s, out_r = np.empty((len(r), count), np.float32), np.empty((len(r), count), np.int64)
            for i in range(len(r)):
                keep = np.flatnonzero(g[i] != r[i])[:count]
                out_s[i], out_r[i] = s[i][keep], g[i][keep]
            return out_s, out_r


N_DOCS, DIM = 120, 16


def _table():
    rng = np.random.default_rng(77)
    vecs = rng.standard_normal((N_DOCS, DIM))
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    t = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(N_DOCS)}
    t["doc 31"] = t["doc 30"]   # an exact duplicate: stays in as a neighbour (only the row id is excluded)
    return t


TABLE = _table()
BARE = (5, 17, 88)              # docs added without an embedding (doc id == i + 1)
GONE = (0, 1, 2, 40, 41, 90)    # deleted after the load: the embedding ids are no longer contiguous


async def _ef(texts):
    return [TABLE[t] for t in texts]


def _kb(path, load=True):
    kb = svs_amd.KB(path, _ef, index_factory=NeighborsOracleIndex)
    if len(kb) == 0:
        with kb.bulk_add_docs() as add_doc:
            for i in range(N_DOCS):
                add_doc(f"doc {i}", no_embedding=i in BARE)
        if load:
            kb.load()
        with kb.bulk_del_docs() as del_doc:
            for i in GONE:
                del_doc(i + 1)
    return kb


def _expected(kb, doc_id, n):
    """numpy over the docs' own vectors: [(score, doc id)] of the n nearest other docs, order (score desc, emb id desc)."""
    with kb.db.transaction():
        rows = kb.db.conn.execute("SELECT embedding, id, text FROM docs WHERE embedding IS NOT NULL ORDER BY embedding").fetchall()
    m = np.array([TABLE[t] for _, _, t in rows], dtype=np.float32)
    me = [i for i, (_, d, _) in enumerate(rows) if d == doc_id][0]
    sc = np.dot(m, m[me])
    order = sorted((i for i in range(len(rows)) if i != me), key=lambda i: (float(sc[i]), rows[i][0]), reverse=True)
    return [(float(sc[i]), rows[i][1]) for i in order[:max(n, 0)]]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _same(got, want):
    """Ids exactly; scores to 1e-6 (the double scores the loaded matrix, tombstoned rows included, with numpy, whose f32
    sums can move by an ulp with the matrix shape -- the GPU tests check bits)."""
    return [d for _, d in got] == [d for _, d in want] and np.allclose([s for s, _ in got], [s for s, _ in want], rtol=0, atol=1e-6)


def _same_graph(got, want):
    return [d for d, _ in got] == [d for d, _ in want] and all(_same(a, b) for (_, a), (_, b) in zip(got, want))


def test_symbol_is_bound():
    assert "svs_index_neighbors" in _native.SIGNATURES
    res, args = _native.SIGNATURES["svs_index_neighbors"]
    assert len(args) == 7


def test_retrieve_similar_maps_doc_to_row_and_back(tmp_path):
    kb = _kb(str(tmp_path / "s.sqlite"))
    for doc in (4, 31, 32, 120):
        got = kb.retrieve_similar(doc, 7)
        assert _same(_got(got), _expected(kb, doc, 7)), doc
        assert doc not in [r["doc"]["id"] for r in got] and len(got) == 7
    assert kb.retrieve_similar(31, 1)[0]["doc"]["id"] == 32 and kb.retrieve_similar(32, 1)[0]["doc"]["id"] == 31
    # shaped like retrieve()
    full = kb.retrieve("doc 9", 1)
    one = kb.retrieve_similar(10, 1)
    assert set(one[0]) == set(full[0]) and set(one[0]["doc"]) == set(full[0]["doc"])
    # counts: everything but the doc itself; nothing
    live = N_DOCS - len(BARE) - len(GONE)
    assert len(kb.retrieve_similar(10, 10 ** 6)) == live - 1
    assert kb.retrieve_similar(10, 0) == []
    kb.close()
    assert OracleIndex.live == 0


def test_retrieve_similar_errors(tmp_path):
    kb = _kb(str(tmp_path / "e.sqlite"))
    with pytest.raises(KeyError) as e:
        kb.retrieve_similar(987654, 3)
    assert e.value.args == (987654,)
    with pytest.raises(KeyError):
        kb.retrieve_similar(GONE[0] + 1, 3)           # deleted
    with pytest.raises(ValueError):
        kb.retrieve_similar(BARE[0] + 1, 3)           # no embedding
    with pytest.raises(KeyError):                     # an embedding id the loaded matrix does not hold
        kb.embeddings_matrix.neighbors([10 ** 9], 3)
    kb.close()


def test_document_neighbors_order_and_ids(tmp_path):
    kb = _kb(str(tmp_path / "g.sqlite"))
    before = NeighborsOracleIndex.calls
    graph = kb.document_neighbors(4)
    assert NeighborsOracleIndex.calls == before + 1   # one native call for the whole graph
    with kb.db.transaction():
        by_emb = [d for d, in kb.db.conn.execute("SELECT id FROM docs WHERE embedding IS NOT NULL ORDER BY embedding")]
    assert [d for d, _ in graph] == by_emb and len(by_emb) == N_DOCS - len(BARE) - len(GONE)
    for doc, nb in graph:
        assert _same(nb, _expected(kb, doc, 4)), doc
        assert all(isinstance(s, float) and isinstance(x, int) for s, x in nb)
    # a list: in the order given, repeats answered each on their own
    some = [77, 4, 120, 4]
    listed = kb.document_neighbors(3, some)
    assert [d for d, _ in listed] == some and all(_same(nb, _expected(kb, d, 3)) for d, nb in listed)
    assert listed[1] == listed[3]
    assert kb.document_neighbors(3, []) == []
    with pytest.raises(KeyError):
        kb.document_neighbors(3, [4, 424242])
    with pytest.raises(ValueError):
        kb.document_neighbors(3, [4, BARE[1] + 1])
    kb.close()


def test_async_twins_equal_sync(tmp_path):
    path = str(tmp_path / "a.sqlite")
    kb = _kb(path)
    docs = [4, 31, 60, 119]
    want = [_got(kb.retrieve_similar(d, 6)) for d in docs]
    want_graph = kb.document_neighbors(5)
    want_some = kb.document_neighbors(2, docs[::-1])
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, _ef, index_factory=NeighborsOracleIndex)
        got = await asyncio.gather(*[akb.retrieve_similar(d, 6) for d in docs])
        graph = await akb.document_neighbors(5)
        some = await akb.document_neighbors(2, docs[::-1])
        with pytest.raises(KeyError):
            await akb.retrieve_similar(424242, 3)
        with pytest.raises(ValueError):
            await akb.retrieve_similar(BARE[2] + 1, 3)
        await akb.close()
        return [_got(g) for g in got], graph, some

    got, graph, some = asyncio.run(run())
    # (the sync KB scored a loaded matrix that still held its tombstoned rows, the async one a freshly built matrix)
    assert all(_same(g, w) for g, w in zip(got, want)) and len(got) == len(want)
    assert _same_graph(graph, want_graph) and _same_graph(some, want_some)
    assert OracleIndex.live == 0


def test_neighbors_parked_across_a_compaction_retries(tmp_path):
    """The call has mapped its ids to rows of the old numbering and is parked in front of the native call; a delete
    compacts the index; the call finds its lookup stale, maps again on a fresh hold and answers in the new numbering."""
    path = str(tmp_path / "r.sqlite")
    kb = _kb(path)
    cache = kb.embeddings_matrix
    first, old_lookup = cache.index, cache._lookup
    ids = [int(e) for e in cache.emb_id_lookup[[100, 60, 101]]]
    entered, go = threading.Event(), threading.Event()
    CompactingOracleIndex.gate = (entered, go)
    out = {}

    def worker():
        try:
            out["res"] = cache.neighbors(ids, 5)
        except BaseException as e:  # noqa: BLE001
            out["err"] = e

    t = threading.Thread(target=worker)
    t.start()
    try:
        assert entered.wait(30)
        before = CompactingOracleIndex.compactions
        with kb.bulk_del_docs() as del_doc:               # 30 more of 120 rows (6 are tombstoned already): past COMPACT_AT
            for i in range(6, 5 + 32):
                if i not in BARE:
                    del_doc(i + 1)
        assert CompactingOracleIndex.compactions == before + 1 and cache.index is first
        assert old_lookup.stale and cache._lookup is not old_lookup
    finally:
        go.set()
        t.join(60)
    assert "err" not in out, out.get("err")
    assert out["res"] == cache.neighbors(ids, 5)
    fresh = svs_amd.KB(path, _ef, index_factory=NeighborsOracleIndex)
    fresh.load()
    assert all(_same(a, b) for a, b in zip(out["res"], fresh.embeddings_matrix.neighbors(ids, 5)))
    kb.close(); fresh.close()
    assert OracleIndex.live == 0

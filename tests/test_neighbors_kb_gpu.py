"""GPU: ``KB.retrieve_similar`` / ``KB.document_neighbors`` and their async twins on a small on-disk KB -- a few hundred
docs, some without an embedding, embedding ids that are no longer contiguous after deletions -- through the real
DeviceIndex (svs_index_neighbors)."""
import asyncio

import numpy as np
import pytest

import svs_amd

pytestmark = pytest.mark.gpu

N_DOCS, DIM = 300, 256
BARE = (7, 123, 250)                                   # added without an embedding (doc id == i + 1)
GONE = tuple(range(40, 60)) + (0, 199, 299)            # deleted after the load: tombstoned rows, gaps in the embedding ids


def _table():
    rng = np.random.default_rng(2024)
    vecs = rng.standard_normal((N_DOCS, DIM))
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    t = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(N_DOCS)}
    t["doc 101"] = t["doc 100"]                        # an exact duplicate
    return t


TABLE = _table()


async def _ef(texts):
    return [TABLE[t] for t in texts]


def _kb(path, dtype="f32"):
    kb = svs_amd.KB(path, _ef, dtype=dtype)
    with kb.bulk_add_docs() as add_doc:
        for i in range(N_DOCS):
            add_doc(f"doc {i}", no_embedding=i in BARE)
    kb.load()
    with kb.bulk_del_docs() as del_doc:
        for i in GONE:
            del_doc(i + 1)
    return kb


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_retrieve_similar_equals_retrieve_with_the_docs_own_text(gpu, tmp_path, dtype):
    kb = _kb(str(tmp_path / "s.sqlite"), dtype)
    assert kb.embeddings_matrix.index.n_masked == len(GONE)      # tombstoned, not rebuilt
    live = N_DOCS - len(BARE) - len(GONE)
    for i in (3, 100, 101, 150, 298):
        doc, n = i + 1, 9
        got = kb.retrieve_similar(doc, n)
        # retrieve() with the doc's own stored text embedding at n + 1, minus the doc.  (The stored row of an f16 index
        # is the half-rounded vector; rounding it again, as retrieve() does with the query, changes nothing.)
        full = [r for r in kb.retrieve(f"doc {i}", n + 1) if r["doc"]["id"] != doc][:n]
        assert _got(got) == _got(full), (dtype, doc)     # (one query, the same kernel, the same query bits: equal)
        assert len(got) == n and set(got[0]) == {"score", "doc"} and got[0]["doc"] == full[0]["doc"]
    assert kb.retrieve_similar(101, 1)[0]["doc"]["id"] == 102 and kb.retrieve_similar(102, 1)[0]["doc"]["id"] == 101
    assert len(kb.retrieve_similar(5, 10 ** 6)) == live - 1 and kb.retrieve_similar(5, 0) == []
    with pytest.raises(KeyError):
        kb.retrieve_similar(10 ** 6, 3)
    with pytest.raises(KeyError):
        kb.retrieve_similar(GONE[0] + 1, 3)
    with pytest.raises(ValueError):
        kb.retrieve_similar(BARE[0] + 1, 3)
    kb.close()


def test_document_neighbors_and_async_twins(gpu, tmp_path):
    path = str(tmp_path / "g.sqlite")
    kb = _kb(path)
    graph = kb.document_neighbors(6)
    with kb.db.transaction():
        by_emb = [d for d, in kb.db.conn.execute("SELECT id FROM docs WHERE embedding IS NOT NULL ORDER BY embedding")]
    assert [d for d, _ in graph] == by_emb and len(graph) == N_DOCS - len(BARE) - len(GONE)
    # per-doc retrieve_similar ids.  (Scores: a doc asked alone takes the single-query kernels, the graph a batched one.)
    for doc, nb in graph:
        one = _got(kb.retrieve_similar(doc, 6))
        assert [d for _, d in nb] == [d for _, d in one], doc
        np.testing.assert_allclose([s for s, _ in nb], [s for s, _ in one], rtol=0, atol=2e-6)
    some = [150, 4, 299, 4]
    listed = kb.document_neighbors(3, some)
    assert [d for d, _ in listed] == some and listed[1] == listed[3]
    with pytest.raises(KeyError):
        kb.document_neighbors(3, [4, 10 ** 6])
    with pytest.raises(ValueError):
        kb.document_neighbors(3, [4, BARE[1] + 1])
    want_one = [_got(kb.retrieve_similar(d, 5)) for d in some]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, _ef)
        one = await asyncio.gather(*[akb.retrieve_similar(d, 5) for d in some])
        g = await akb.document_neighbors(6)
        ls = await akb.document_neighbors(3, some)
        with pytest.raises(KeyError):
            await akb.retrieve_similar(10 ** 6, 3)
        with pytest.raises(ValueError):
            await akb.retrieve_similar(BARE[2] + 1, 3)
        await akb.close()
        return [_got(x) for x in one], g, ls

    one, g, ls = asyncio.run(run())
    # (the async KB built its matrix from the live rows; the sync one held tombstones: same rows, same kernels per row)
    assert [[d for _, d in x] for x in one] == [[d for _, d in x] for x in want_one]
    assert [(d, [x for _, x in nb]) for d, nb in g] == [(d, [x for _, x in nb]) for d, nb in graph]
    assert [(d, [x for _, x in nb]) for d, nb in ls] == [(d, [x for _, x in nb]) for d, nb in listed]
    for (_, a), (_, b) in zip(g, graph):
        np.testing.assert_allclose([s for s, _ in a], [s for s, _ in b], rtol=0, atol=2e-6)

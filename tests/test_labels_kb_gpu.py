"""GPU: ``KB.retrieve_at_level`` / ``AsyncKB.retrieve_at_level`` on a real index -- the level of every doc stored as a
label beside its vector, the filter run on the device.  Held against ``retrieve_within`` with the level's doc ids
(scores and doc ids, exactly: both end in the same score and top-k kernels), through appends with the column installed,
an in-place compaction, and a fresh index generation."""
import asyncio

import numpy as np
import pytest

import svs_amd

pytestmark = pytest.mark.gpu

D = 64


def _unit(rng, n, d=D):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _embedder(seed, n_texts):
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(n_texts)] + [f"q {i}" for i in range(4)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts)))}

    async def ef(ts):
        return [table[t] for t in ts]

    return ef


def _fill(add_doc, level, start, n_roots):
    """n_roots roots with 3 children each and 2 grandchildren per child (10 docs per root); returns the next text number."""
    i = start
    for _ in range(n_roots):
        root = add_doc(f"doc {i}"); level[root] = 0; i += 1
        for _ in range(3):
            child = add_doc(f"doc {i}", parent_id=root); level[child] = 1; i += 1
            for _ in range(2):
                leaf = add_doc(f"doc {i}", parent_id=child); level[leaf] = 2; i += 1
    return i


def _pairs(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _agree(kb, level, tag):
    for levels in (0, 1, 2, (0, 2), 5):
        ls = {levels} if isinstance(levels, int) else set(levels)
        ids = [d for d, lv in level.items() if lv in ls]
        for q, n in (("q 0", 10), ("q 1", len(ids) + 3)):
            got = kb.retrieve_at_level(q, n, levels)
            want = kb.retrieve_within(q, n, ids) if ids else []
            assert _pairs(got) == _pairs(want), (tag, levels, q, n)
            assert len(got) == min(n, len(ids)) and {r["doc"]["level"] for r in got} <= ls, (tag, levels)


def test_retrieve_at_level_follows_the_kb(gpu, tmp_path):
    ef = _embedder(3, 500)
    kb = svs_amd.KB(str(tmp_path / "kb.sqlite"), ef)
    level = {}
    with kb.bulk_add_docs() as add_doc:
        nxt = _fill(add_doc, level, 0, 30)                      # 300 docs
    kb.load()
    first = kb.embeddings_matrix.index
    assert not first.labels().any()                             # lazily: no column before the first labelled retrieval
    _agree(kb, level, "fresh")
    with kb.db.transaction():
        emb_level = sorted(kb.db.conn.execute("SELECT embedding, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    assert first.labels().tolist() == [lv + 1 for _, lv in emb_level]      # the stored label is level + 1
    # docs on two levels, added with the column installed
    roots = [d for d, lv in level.items() if lv == 0]
    with kb.bulk_add_docs() as add_doc:
        for j in range(4):
            level[add_doc(f"doc {nxt}")] = 0; nxt += 1
            level[add_doc(f"doc {nxt}", parent_id=roots[j])] = 1; nxt += 1
    assert kb.embeddings_matrix.index is first and first.n == 308
    assert first.labels(300, 8).tolist() == [1, 2] * 4
    _agree(kb, level, "appended")
    # enough deletions for the in-place compaction: the labels move with the rows
    gone = [d for d, lv in level.items() if lv == 2][::2] + [d for d, lv in level.items() if lv == 0 and d not in roots]
    with kb.bulk_del_docs() as del_doc:
        for d in gone:
            del_doc(d)
    for d in gone:
        del level[d]
    assert kb.embeddings_matrix.index is first and first.n == 308 - len(gone) and first.n_masked == 0
    _agree(kb, level, "compacted")
    # a fresh generation installs its own column
    kb.embeddings_matrix.invalidate()
    _agree(kb, level, "rebuilt")
    assert kb.embeddings_matrix.index is not first
    path = kb.db.path
    want = [_pairs(kb.retrieve_at_level("q 2", 12, lv)) for lv in (0, 1, 2, (0, 2), 5)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef)
        got = await asyncio.gather(*[akb.retrieve_at_level("q 2", 12, lv) for lv in (0, 1, 2, (0, 2), 5)])
        await akb.close()
        return [_pairs(r) for r in got]

    assert asyncio.run(run()) == want

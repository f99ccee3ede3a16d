"""GPU: ``KB.retrieve_under`` / ``AsyncKB.retrieve_under`` on a real index -- the parent of every doc stored as
``parent_id + 1`` in column 1 beside its vector (the level in column 0), the conjunction run on the device.  Held
against ``retrieve_within`` with the children's doc ids (scores and doc ids, exactly: both end in the same score and
top-k kernels), through appends with the columns installed, an in-place compaction, and a fresh index generation."""
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


def _fill(add_doc, parent, level, start, n_roots):
    """n_roots roots with 3 children each and 2 grandchildren per child (10 docs per root); returns the next text number."""
    i = start
    for _ in range(n_roots):
        root = add_doc(f"doc {i}"); parent[root], level[root] = None, 0; i += 1
        for _ in range(3):
            child = add_doc(f"doc {i}", parent_id=root); parent[child], level[child] = root, 1; i += 1
            for _ in range(2):
                leaf = add_doc(f"doc {i}", parent_id=child); parent[leaf], level[leaf] = child, 2; i += 1
    return i


def _pairs(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _asks(parent, level):
    """(parent_ids, levels): one parent, several parents, a parent without children, with levels."""
    roots = [d for d, lv in level.items() if lv == 0]
    mids = [d for d, lv in level.items() if lv == 1]
    leaf = next(d for d, lv in level.items() if lv == 2)
    return [(roots[0], None), (mids[1], None), (roots[:7] + mids[3:40:4], None), (leaf, None), ([leaf, 10 ** 6], None),
            (roots[:7] + mids[3:40:4], 2), (roots + mids, (1,)), (roots[2:5], [0, 2]), ([], None)]


def _agree(kb, parent, level, tag):
    for parents, levels in _asks(parent, level):
        ps = {parents} if isinstance(parents, int) else set(parents)
        ls = None if levels is None else {levels} if isinstance(levels, int) else set(levels)
        ids = [d for d, p in parent.items() if p in ps and (ls is None or level[d] in ls)]
        for q, n in (("q 0", 10), ("q 1", len(ids) + 3)):
            got = kb.retrieve_under(q, n, parents, levels)
            want = kb.retrieve_within(q, n, ids) if ids else []
            assert _pairs(got) == _pairs(want), (tag, parents, levels, q, n)
            assert len(got) == min(n, len(ids)) and {r["doc"]["parent_id"] for r in got} <= ps, (tag, parents, levels)


def test_retrieve_under_follows_the_kb(gpu, tmp_path):
    ef = _embedder(4, 500)
    kb = svs_amd.KB(str(tmp_path / "kb.sqlite"), ef)
    parent, level = {}, {}
    with kb.bulk_add_docs() as add_doc:
        nxt = _fill(add_doc, parent, level, 0, 30)              # 300 docs
    kb.load()
    first = kb.embeddings_matrix.index
    base = first.hbm_bytes
    assert not first.column(1).any() and not first.labels().any()          # lazily: no column before the first such retrieval
    assert len(kb.retrieve_under("q 0", 3, next(iter(level)))) == 3
    one = first.hbm_bytes
    assert one >= base + 4 * 300 and not first.labels().any()              # column 1 alone: no level was named
    _agree(kb, parent, level, "fresh")
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, parent_id, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    assert first.column(1).tolist() == [0 if p is None else p + 1 for _, p, _ in by_emb]      # parent_id + 1, 0: no parent
    assert first.labels().tolist() == [lv + 1 for _, _, lv in by_emb]
    # docs on two levels, added with both columns installed
    roots = [d for d, lv in level.items() if lv == 0]
    with kb.bulk_add_docs() as add_doc:
        for j in range(4):
            d0 = add_doc(f"doc {nxt}"); parent[d0], level[d0] = None, 0; nxt += 1
            d1 = add_doc(f"doc {nxt}", parent_id=roots[j]); parent[d1], level[d1] = roots[j], 1; nxt += 1
    assert kb.embeddings_matrix.index is first and first.n == 308
    assert first.column(1, 300, 8).tolist() == [v for j in range(4) for v in (0, roots[j] + 1)]
    assert first.labels(300, 8).tolist() == [1, 2] * 4
    assert len(kb.retrieve_under("q 0", 10, roots[0])) == 4                 # three children, and the new one
    _agree(kb, parent, level, "appended")
    # enough deletions for the in-place compaction: the values move with the rows
    gone = [d for d, lv in level.items() if lv == 2][::2] + [d for d, lv in level.items() if lv == 0 and d not in roots]
    with kb.bulk_del_docs() as del_doc:
        for d in gone:
            del_doc(d)
    for d in gone:
        del parent[d], level[d]
    assert kb.embeddings_matrix.index is first and first.n == 308 - len(gone) and first.n_masked == 0
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, parent_id FROM docs WHERE embedding IS NOT NULL").fetchall())
    assert first.column(1).tolist() == [0 if p is None else p + 1 for _, p in by_emb]
    _agree(kb, parent, level, "compacted")
    # a fresh generation installs its own columns
    kb.embeddings_matrix.invalidate()
    _agree(kb, parent, level, "rebuilt")
    assert kb.embeddings_matrix.index is not first
    path = kb.db.path
    asks = _asks(parent, level)
    want = [_pairs(kb.retrieve_under("q 2", 12, p, lv)) for p, lv in asks]
    assert any(want) and not all(want)
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef)
        got = await asyncio.gather(*[akb.retrieve_under("q 2", 12, p, lv) for p, lv in asks])
        await akb.close()
        return [_pairs(r) for r in got]

    assert asyncio.run(run()) == want

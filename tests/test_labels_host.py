"""CPU: labelled retrieval above the kernel -- emb id <-> row <-> doc mapping of ``KB.retrieve_at_level`` /
``AsyncKB.retrieve_at_level`` and the label column's bookkeeping in ``DeviceEmbeddingsMatrix`` (lazy install once per
index generation, appends with and without labels), through a numpy double of DeviceIndex whose ``set_labels`` /
``search_labeled`` are the plain numpy model of the definition; and the new kernels' resource report."""
import asyncio
import logging
import os

import numpy as np
import pytest

from fake_backend import OracleIndex
from oracle import svs_oracle as oracle
from test_kernel_resources import RES, _demangle, _resources

import svs_amd
from svs_amd import multi as multi_mod
from svs_amd.kb import embedding_to_bytes


class LabelOracleIndex(OracleIndex):
    """OracleIndex with a label column: state [matrix, dead mask, labels], shared by every owner like the HBM copy."""

    dtype = "f32"
    set_calls = []      # (row0, number of labels) of every set_labels call, all instances

    def __init__(self, matrix, device=0, row_offset=0, _shared=None):
        super().__init__(matrix, device, row_offset, _shared=_shared)
        if len(self._st) == 2:
            self._st.append(np.zeros(self.n, dtype=np.uint32))

    def share(self):
        self._check()
        return LabelOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def append(self, rows):
        super().append(rows)
        self._st[2] = np.concatenate([self._st[2], np.zeros(self.n - len(self._st[2]), dtype=np.uint32)])

    def set_labels(self, labels, row0=None):
        self._check()
        lab = np.asarray(labels, dtype=np.uint32).reshape(-1)
        r0 = 0 if row0 is None else int(row0) - self.row_offset
        if r0 < 0 or r0 + len(lab) > self.n:
            raise ValueError("rows outside the index")
        LabelOracleIndex.set_calls.append((r0, len(lab)))
        self._st[2][r0:r0 + len(lab)] = lab

    def search_labeled(self, q, n, labels):
        self._check()
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        S = np.flatnonzero(np.isin(self._st[2], np.asarray(list(labels), dtype=np.uint32)) & ~self._st[1])
        top = oracle.total_order_top_k(oracle.cpu_scores(self._m[S], q), min(max(n, 0), len(S))) if len(S) else []
        return [(s, int(S[p]) + self.row_offset) for s, p in top], len(S)

    def search_within(self, q, n, rows):
        self._check()
        S = np.unique(np.asarray(rows, dtype=np.int64)) - self.row_offset
        S = S[~self._st[1][S]]
        top = oracle.total_order_top_k(oracle.cpu_scores(self._m[S], np.asarray(q, dtype=np.float32)), min(max(n, 0), len(S))) if len(S) else []
        return [(s, int(S[p]) + self.row_offset) for s, p in top]


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_roots=10, d=16, seed=21):
    """A three-level KB: n_roots roots, 3 children each, 2 grandchildren per child.  {doc id: level}."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(6)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=LabelOracleIndex)
    level, i = {}, 0
    with kb.bulk_add_docs() as add_doc:
        for _ in range(n_roots):
            root = add_doc(f"doc {i}"); level[root] = 0; i += 1
            for _ in range(3):
                child = add_doc(f"doc {i}", parent_id=root); level[child] = 1; i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); level[leaf] = 2; i += 1
    return kb, ef, table, level


def _expected(kb, table, query, n, levels):
    """The model over the docs' own vectors: [(score, doc id)] of the docs on ``levels``, rows in embedding-id order."""
    with kb.db.transaction():
        rows = kb.db.conn.execute("SELECT embedding, id, text, level FROM docs WHERE embedding IS NOT NULL").fetchall()
    rows = sorted(r for r in rows if r[3] in levels)
    if not rows:
        return []
    m = np.array([table[t] for _, _, t, _ in rows], dtype=np.float32)
    top = oracle.total_order_top_k(oracle.cpu_scores(m, np.array(table[query], dtype=np.float32)), min(n, len(rows)))
    return [(s, rows[p][1]) for s, p in top]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_retrieve_at_level_maps_rows_to_docs(tmp_path, caplog):
    kb, ef, table, level = _kb(tmp_path, "a.sqlite")
    on = {L: [d for d, lv in level.items() if lv == L] for L in range(3)}
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_at_level("q 0", 7, 1)
    assert _got(got) == _expected(kb, table, "q 0", 7, {1}) and len(got) == 7
    assert {r["doc"]["level"] for r in got} == {1}
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 7 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(on[1])} cosine similarities", "retrieved top 7 documents"]
    # same result shape as retrieve(); the same answer as retrieve_within over the level's doc ids
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])
    for levels in (0, 1, 2, (0, 2), [2, 2, 1], np.int64(1), range(3)):
        ls = {int(levels)} if isinstance(levels, (int, np.integer)) else set(levels)
        ids = [d for d, lv in level.items() if lv in ls]
        got = kb.retrieve_at_level("q 1", 500, levels)
        assert _got(got) == _expected(kb, table, "q 1", 500, ls) == _got(kb.retrieve_within("q 1", 500, ids))
        assert len(got) == len(ids)
    assert kb.retrieve_at_level("q 1", 5, 3) == [] and kb.retrieve_at_level("q 1", 5, []) == []
    assert kb.retrieve_at_level("q 1", 0, 1) == []
    # the stored label is level + 1, in embedding-id order
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    assert kb.embeddings_matrix.index._st[2].tolist() == [lv + 1 for _, lv in by_emb]
    kb.close()
    assert OracleIndex.live == 0


def test_level_arguments_are_checked(tmp_path):
    kb, ef, table, level = _kb(tmp_path, "v.sqlite", n_roots=2)
    for bad in (-1, [0, -2], 1.0, [True], "1", range(1025)):
        with pytest.raises(ValueError):
            kb.retrieve_at_level("q 0", 3, bad)
    assert len(kb.retrieve_at_level("q 0", 3, range(1024))) == 3      # 1,024 distinct levels are allowed

    async def run():
        akb = svs_amd.AsyncKB(kb.db.path, ef, index_factory=LabelOracleIndex)
        for bad in (-1, range(1025)):
            with pytest.raises(ValueError):
                await akb.retrieve_at_level("q 0", 3, bad)
        await akb.close()

    asyncio.run(run())
    kb.close()


def test_the_column_is_installed_once_per_generation_and_follows_appends(tmp_path):
    kb, ef, table, level = _kb(tmp_path, "g.sqlite")
    LabelOracleIndex.set_calls.clear()
    kb.load()
    kb.retrieve("q 0", 3)
    kb.retrieve_within("q 0", 3, list(level)[:5])
    assert LabelOracleIndex.set_calls == []                      # lazily: nothing before the first labelled retrieval
    n = len(level)
    kb.retrieve_at_level("q 0", 3, 1)
    assert LabelOracleIndex.set_calls == [(0, n)]                # one call, the whole range
    kb.retrieve_at_level("q 2", 3, (0, 2))
    assert LabelOracleIndex.set_calls == [(0, n)]
    first = kb.embeddings_matrix.index
    # bulk_add_docs with the column installed: the new rows' labels go in behind the append, nothing is re-installed
    root = next(d for d, lv in level.items() if lv == 0)
    child = next(d for d, lv in level.items() if lv == 1)
    table["late root"], table["late leaf"] = table["q 3"], table["q 4"]
    with kb.bulk_add_docs() as add_doc:
        a = add_doc("late root")
        b = add_doc("late leaf", parent_id=child)
        add_doc("doc 399", parent_id=root, no_embedding=True)
    level[a], level[b] = 0, 2
    assert kb.embeddings_matrix.index is first and LabelOracleIndex.set_calls == [(0, n), (n, 2)]
    assert first._st[2][n:].tolist() == [1, 3]
    assert [r["doc"]["id"] for r in kb.retrieve_at_level("q 3", 1, 0)] == [a]
    assert [r["doc"]["id"] for r in kb.retrieve_at_level("q 4", 1, 2)] == [b]
    assert kb.retrieve_at_level("q 4", 500, 1) == kb.retrieve_within("q 4", 500, [d for d, lv in level.items() if lv == 1])
    assert LabelOracleIndex.set_calls == [(0, n), (n, 2)]
    # deletions: the tombstoned rows drop out
    with kb.bulk_del_docs() as del_doc:
        del_doc(a)
    del level[a]
    assert _got(kb.retrieve_at_level("q 3", 500, 0)) == _expected(kb, table, "q 3", 500, {0})
    # an append WITHOUT labels: the column counts as not installed, and the next labelled retrieval installs all of it
    table["bare"] = table["q 5"]
    with kb.db.transaction():
        doc, lv = kb.db.add_doc_at("bare", child, None)
        emb = kb.db.set_doc_embedding(doc, embedding_to_bytes(table["bare"]))
    assert lv == 2
    assert kb.embeddings_matrix.append(np.array([table["bare"]], dtype=np.float32), [emb])
    assert first._st[2][-1] == 0 and len(LabelOracleIndex.set_calls) == 2
    assert [r["doc"]["id"] for r in kb.retrieve_at_level("q 5", 1, 2)] == [doc]
    assert LabelOracleIndex.set_calls[2:] == [(0, n + 3)] and first._st[2][-1] == 3
    kb.retrieve_at_level("q 5", 1, 2)
    assert len(LabelOracleIndex.set_calls) == 3
    # a fresh generation installs its own column, once
    kb.embeddings_matrix.invalidate()
    level[doc] = 2
    assert _got(kb.retrieve_at_level("q 5", 500, 2)) == _expected(kb, table, "q 5", 500, {2})
    assert kb.embeddings_matrix.index is not first
    live = n + 3 - 1                                             # (the deleted doc's embedding is gone from storage)
    assert LabelOracleIndex.set_calls[3:] == [(0, live)]
    kb.retrieve_at_level("q 5", 5, 0)
    assert len(LabelOracleIndex.set_calls) == 4
    kb.close()
    assert OracleIndex.live == 0


def test_async_retrieve_at_level_equals_sync(tmp_path, caplog):
    kb, ef, table, level = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    asks = [("q 0", 5, 0), ("q 1", 9, 1), ("q 2", 500, 2), ("q 3", 4, (0, 2)), ("q 4", 3, 7)]
    want = [_got(kb.retrieve_at_level(*a)) for a in asks]
    assert [len(w) for w in want] == [5, 9, 60, 4, 0]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=LabelOracleIndex)
        LabelOracleIndex.set_calls.clear()
        got = await asyncio.gather(*[akb.retrieve_at_level(*a) for a in asks])
        assert LabelOracleIndex.set_calls == [(0, len(level))]   # five concurrent tasks, one installation
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_at_level("q 1", 9, 1)
        async with akb.bulk_add_docs() as add_doc:
            table["late"] = table["q 5"]
            new = await add_doc("late")
        late = await akb.retrieve_at_level("q 5", 1, 0)
        assert [r["doc"]["id"] for r in late] == [new] and LabelOracleIndex.set_calls[1:] == [(len(level), 1)]
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 9 documents with query string: q 1", "got embedding for query!",
                     "computed 30 cosine similarities", "retrieved top 9 documents"]
    assert OracleIndex.live == 0


def test_multi_and_sharded_labelled_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[LabelOracleIndex(m[:20], 0, 0), LabelOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError):
        mi.search_labeled(m[0], 3, [1])
    with pytest.raises(NotImplementedError):
        mi.search_batch_labeled(m[:2], 3, [1])
    with pytest.raises(NotImplementedError):
        mi.set_labels(np.ones(40, dtype=np.uint32))
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError):
        ShardedIndex.search_labeled(None, m[0], 3, [1])


def test_label_kernels_use_no_scratch():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    names = _demangle([n for n in table if "label_" in n])
    for kernel, instances in (("label_count_kernel", 1), ("label_scan_kernel", 1), ("label_write_kernel", 2), ("label_map_rows_kernel", 1)):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == instances, (kernel, sorted(names.values()))
        for h in hits:
            r = table[h]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{kernel}: {r}"
    # none is a score kernel by name: test_kernel_resources.py enumerates those (no new gather instantiation)
    assert not [p for p in names.values() if "gemv_" in p or "gemm_" in p or "gather_scores_kernel" in p]

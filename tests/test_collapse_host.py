"""CPU: collapsed retrieval above the kernel -- parent <-> column value, emb id <-> row <-> doc mapping of
``KB.retrieve_collapsed`` / ``AsyncKB.retrieve_collapsed`` through a numpy double of DeviceIndex whose
``search_collapsed`` is the numpy model of the definition (collapse_model.py); the column shared with
``retrieve_under``; ``collapsed_op``; the multi-device refusals; and the new kernels' resource report."""
import asyncio
import logging
import os
import re

import numpy as np
import pytest

import collapse_model
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources
from where_backend import ColumnOracleIndex

import svs_amd
from svs_amd import _native, index as index_mod, kb as kb_mod, multi as multi_mod


class CollapseOracleIndex(ColumnOracleIndex):
    """ColumnOracleIndex whose ``search_collapsed`` is the model over its own state."""

    calls = []          # (n, column, zero) of every search_collapsed call, all instances

    def share(self):
        self._check()
        return CollapseOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_collapsed(self, q, n, column, zero="single"):
        self._check()
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        CollapseOracleIndex.calls.append((n, column, zero))
        single = index_mod.collapse_zero_mode(zero) == _native.COLLAPSE_ZERO_SINGLE
        s, r, v, groups = collapse_model.collapsed(self.scores(q), self._st[2][column], self._st[1], single, n)
        return list(zip(s.astype(np.float64).tolist(), (r + self.row_offset).tolist(), v.tolist())), groups


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_roots=8, d=16, seed=41):
    """A three-level KB: n_roots roots, 3 children each, 2 grandchildren per child; the last root has no child.
    {doc id: parent id or None}."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=CollapseOracleIndex)
    parent, i = {}, 0
    with kb.bulk_add_docs() as add_doc:
        for r in range(n_roots):
            root = add_doc(f"doc {i}"); parent[root] = None; i += 1
            for _ in range(3 if r < n_roots - 1 else 0):
                child = add_doc(f"doc {i}", parent_id=root); parent[child] = root; i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); parent[leaf] = child; i += 1
    return kb, ef, table, parent


def _expected(kb, table, query, n):
    """The definition over the docs' own vectors: every parent is represented by its child with the highest (score,
    embedding id), a doc without a parent by itself; [(score, doc id)] of the n best representatives."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text, parent_id FROM docs WHERE embedding IS NOT NULL").fetchall())
    m = np.array([table[t] for _, _, t, _ in rows], dtype=np.float32)
    s = np.dot(m, np.array(table[query], dtype=np.float32))
    best = {}
    for i, (_, doc, _, par) in enumerate(rows):
        g = ("doc", doc) if par is None else ("parent", par)
        best[g] = max(best.get(g, (-np.inf, -1)), (s[i], i))
    top = sorted(best.values(), reverse=True)[:max(n, 0)]
    return [(float(sc), rows[i][1]) for sc, i in top]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_retrieve_collapsed_keeps_one_document_per_parent(tmp_path, caplog):
    kb, ef, table, parent = _kb(tmp_path, "a.sqlite")
    CollapseOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_collapsed("q 0", 5)
    assert _got(got) == _expected(kb, table, "q 0", 5) and len(got) == 5
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 5 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(parent)} cosine similarities", "retrieved top 5 documents"]
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])      # retrieve's shape
    assert got[0]["doc"]["id"] == full[0]["doc"]["id"]                                      # the best doc is always in W
    assert CollapseOracleIndex.calls == [(5, kb_mod.PARENT_COLUMN, "single")]
    # every n: 8 roots stand for themselves, 7 roots and 21 children are parents -> 36 groups
    groups = 8 + 7 + 21
    for q, n in (("q 1", 1), ("q 1", 12), ("q 2", groups), ("q 2", 500), ("q 3", 0), ("q 3", -2)):
        got = kb.retrieve_collapsed(q, n)
        assert _got(got) == _expected(kb, table, q, n) and len(got) == min(max(n, 0), groups), (q, n)
        seen = [("doc", r["doc"]["id"]) if r["doc"]["parent_id"] is None else ("parent", r["doc"]["parent_id"]) for r in got]
        assert len(set(seen)) == len(seen)                                                  # at most one per parent
        assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)
    # a parent that holds the best documents still yields one: the children of one child doc are copies of the query
    child = next(d for d, p in parent.items() if p is not None and parent[p] is None)
    table["twin a"] = table["twin b"] = table["twin c"] = table["q 4"]
    with kb.bulk_add_docs() as add_doc:
        twins = [add_doc(t, parent_id=child) for t in ("twin a", "twin b", "twin c")]
    got = kb.retrieve_collapsed("q 4", 4)
    assert _got(got) == _expected(kb, table, "q 4", 4)
    assert got[0]["doc"]["id"] == twins[-1] and not {r["doc"]["id"] for r in got[1:]} & set(twins)   # (the tie: the later embedding)
    assert [r["doc"]["id"] for r in kb.retrieve("q 4", 3)] == twins[::-1]                   # what over-fetching would have to undo
    # deletions: the representative dies, the runner-up takes over; a parent whose children are all gone disappears
    with kb.bulk_del_docs() as del_doc:
        del_doc(twins[-1])
    got = kb.retrieve_collapsed("q 4", 4)
    exp = _expected(kb, table, "q 4", 4)
    # (the double still holds the tombstoned row, so its matrix product has another shape than the expectation's: the
    #  docs must be equal, the scores agree to f32 rounding)
    assert got[0]["doc"]["id"] == twins[1] and [d for _, d in _got(got)] == [d for _, d in exp]
    assert [s for s, _ in _got(got)] == pytest.approx([s for s, _ in exp], abs=1e-6)
    kb.close()
    assert OracleIndex.live == 0


def test_the_parent_column_is_shared_with_retrieve_under(tmp_path):
    kb, ef, table, parent = _kb(tmp_path, "g.sqlite")
    calls = ColumnOracleIndex.set_calls
    calls.clear()
    n = len(parent)
    root = next(d for d, p in parent.items() if p is None)
    kb.retrieve("q 0", 3)
    assert calls == []                                           # lazily: nothing before the first retrieval that needs it
    kb.retrieve_collapsed("q 0", 3)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, n)]               # installed through ensure_column, once, the whole range
    kb.retrieve_under("q 0", 3, root)
    kb.retrieve_collapsed("q 1", 3)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, n)]
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, parent_id FROM docs WHERE embedding IS NOT NULL").fetchall())
    st = kb.embeddings_matrix.index._st[2]
    assert st[kb_mod.PARENT_COLUMN].tolist() == [0 if p is None else p + 1 for _, p in by_emb] and not st[0].any()
    # the other way round on a fresh KB: retrieve_under installs, retrieve_collapsed finds the column
    kb2, _, table2, parent2 = _kb(tmp_path, "h.sqlite", n_roots=3)
    calls.clear()
    kb2.retrieve_under("q 0", 3, next(d for d, p in parent2.items() if p is None))
    assert _got(kb2.retrieve_collapsed("q 0", 4)) == _expected(kb2, table2, "q 0", 4)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, len(parent2))]
    # bulk_add_docs passes the new rows' values behind the append: nothing is re-installed
    table2["late"] = table2["q 5"]
    with kb2.bulk_add_docs() as add_doc:
        late = add_doc("late")
    assert kb2.retrieve_collapsed("q 5", 1)[0]["doc"]["id"] == late
    assert calls[1:] == [(kb_mod.PARENT_COLUMN, len(parent2), 1)]          # (the level column was never installed)
    kb.close()
    kb2.close()
    assert OracleIndex.live == 0


def test_arguments_are_checked():
    assert index_mod.collapse_zero_mode("single") == _native.COLLAPSE_ZERO_SINGLE == 1
    assert index_mod.collapse_zero_mode("group") == _native.COLLAPSE_ZERO_IS_GROUP == 0
    for bad in ("", "zero", None, 1, True, b"single"):
        with pytest.raises(ValueError):
            index_mod.collapse_zero_mode(bad)
    q = np.zeros(4, dtype=np.float32)
    # the column and the zero mode are checked before the handle is touched
    for bad in (-1, 4, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            index_mod.DeviceIndex.search_batch_collapsed(SimpleQueries(), q[None, :], 3, bad)
    with pytest.raises(ValueError):
        index_mod.DeviceIndex.search_batch_collapsed(SimpleQueries(), q[None, :], 3, 1, "both")
    with pytest.raises(ValueError):
        index_mod.DeviceIndex.search_collapsed(SimpleQueries(), q[None, :], 3, 1)           # a 2-D query
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svs_amd.h")).read()
    assert "SVS_COLLAPSE_ZERO_IS_GROUP = 0, SVS_COLLAPSE_ZERO_SINGLE = 1" in hdr


class SimpleQueries:
    """What DeviceIndex.search_batch_collapsed touches before its argument checks."""

    @staticmethod
    def _queries_2d(q):
        return np.ascontiguousarray(q, dtype=np.float32)


def test_async_retrieve_collapsed_equals_sync(tmp_path, caplog):
    kb, ef, table, parent = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    asks = [("q 0", 5), ("q 1", 1), ("q 2", 36), ("q 3", 500), ("q 4", 0), ("q 5", 9)]
    want = [_got(kb.retrieve_collapsed(*a)) for a in asks]
    assert [len(w) for w in want] == [5, 1, 36, 36, 0, 9]
    assert want == [_expected(kb, table, *a) for a in asks]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=CollapseOracleIndex)
        ColumnOracleIndex.set_calls.clear()
        got = await asyncio.gather(*[akb.retrieve_collapsed(*a) for a in asks])
        assert ColumnOracleIndex.set_calls == [(kb_mod.PARENT_COLUMN, 0, len(parent))]    # six concurrent tasks, one installation
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_collapsed("q 1", 9)
        root = next(d for d, p in parent.items() if p is None)
        async with akb.bulk_add_docs() as add_doc:
            table["late"] = table["q 6"]
            new = await add_doc("late", parent_id=root)
        late = await akb.retrieve_collapsed("q 6", 2)
        assert late[0]["doc"]["id"] == new and late[1]["doc"]["parent_id"] != root
        under = await akb.retrieve_under("q 6", 1, root)                                    # the same column
        # (+ the append's values for the one installed column; retrieve_under installed nothing)
        assert under[0]["doc"]["id"] == new and ColumnOracleIndex.set_calls[1:] == [(kb_mod.PARENT_COLUMN, len(parent), 1)]
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 9 documents with query string: q 1", "got embedding for query!",
                     f"computed {len(parent)} cosine similarities", "retrieved top 9 documents"]
    assert OracleIndex.live == 0


def test_multi_and_sharded_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[CollapseOracleIndex(m[:20], 0, 0), CollapseOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError):
        mi.search_collapsed(m[0], 3, 1)
    with pytest.raises(NotImplementedError):
        mi.search_batch_collapsed(m[:2], 3, 1)
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError):
        ShardedIndex.search_collapsed(None, m[0], 3, 1)
    with pytest.raises(NotImplementedError):
        ShardedIndex.search_batch_collapsed(None, m[:2], 3, 1)


def test_collapsed_op_maps_rows_to_embedding_ids():
    from svs_amd.matrix import collapsed_op
    m = _unit(np.random.default_rng(2), 30, 8)
    idx = CollapseOracleIndex(m, 0, 100)
    idx.set_column(2, np.arange(30) // 4, 100)                   # rows 0 .. 3 carry 0, then groups of four
    arr = np.arange(30, dtype=np.int64) * 7 + 5                  # row r holds embedding id 7 r + 5
    for zero, groups in (("single", 4 + 7), ("group", 8)):
        native, finish = collapsed_op(m[9], 6, 2, zero)
        used, (hits, g) = native(idx, None)
        assert used is idx and len(hits) == 6 and g == groups
        assert all(100 <= r < 130 for _, r, _ in hits)
        out, og = finish((used, (hits, g)), arr)
        assert og == groups and out == [(s, 7 * (r - 100) + 5, v) for s, r, v in hits]
        assert out[0][1] == 7 * 9 + 5 and out[0][2] == 9 // 4 and all(isinstance(x, int) for o in out for x in o[1:])
    native, finish = collapsed_op(m[9], 6, 2)                    # the default: "single"
    assert native(idx, None)[1][1] == 11
    idx.release()


def test_collapse_kernels_use_no_scratch_and_no_lds():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    names = _demangle([n for n in table if "collapse_" in n])
    with open(RES) as f:
        txt = f.read()
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)}
    # the groups live in HBM and the survivors are counted with a ballot: none of the three kernels needs LDS
    for kernel in ("collapse_reduce_kernel", "collapse_mark_kernel", "collapse_values_kernel"):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == 1, (kernel, sorted(names.values()))
        r = table[hits[0]]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{kernel}: {r}"
        assert lds[hits[0]] == 0, (kernel, lds[hits[0]])
    assert len(names) == 3, sorted(names.values())

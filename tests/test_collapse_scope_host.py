"""CPU: the scoped collapsed search above the kernels -- ``KB.retrieve_collapsed(..., levels=...)`` and its async twin
through a numpy double of DeviceIndex whose ``search_collapsed_where`` / ``search_collapsed_within`` are the numpy model
of the definition (collapse_scope_model.py); the two columns they install; the argument checks that precede the
handle; the matrix ops; the multi-device refusals; the header's prototypes; and the new kernels' resource report."""
import asyncio
import logging
import os
import re

import numpy as np
import pytest

import collapse_model
import collapse_scope_model
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources
from where_backend import COLUMNS, ColumnOracleIndex
from where_model import where_mask

import svs_amd
from svs_amd import _native, index as index_mod, kb as kb_mod, multi as multi_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ScopedOracleIndex(ColumnOracleIndex):
    """ColumnOracleIndex whose collapsed searches, scoped and unscoped, are the models over its own state."""

    calls = []          # (entry, n, scope, column, zero) of every collapsed call, all instances

    def share(self):
        self._check()
        return ScopedOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def _query(self, q, n):
        self._check()
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        return q

    def search_collapsed(self, q, n, column, zero="single"):
        q = self._query(q, n)
        ScopedOracleIndex.calls.append(("collapsed", n, None, column, zero))
        single = index_mod.collapse_zero_mode(zero) == _native.COLLAPSE_ZERO_SINGLE
        s, r, v, groups = collapse_model.collapsed(self.scores(q), self._st[2][column], self._st[1], single, n)
        return list(zip(s.astype(np.float64).tolist(), (r + self.row_offset).tolist(), v.tolist())), groups

    def _scoped(self, q, n, in_scope, column, zero):
        single = index_mod.collapse_zero_mode(zero) == _native.COLLAPSE_ZERO_SINGLE
        s, r, v, groups, matched = collapse_scope_model.collapsed_scoped(self.scores(q), self._st[2][column], self._st[1], in_scope, single, n)
        return list(zip(s.astype(np.float64).tolist(), (r + self.row_offset).tolist(), v.tolist())), groups, matched

    def search_collapsed_where(self, q, n, where, column, zero="single"):
        q = self._query(q, n)
        where = [(c, op, list(arg) if op in ("in", "not in") else arg) for c, op, arg in where]
        ScopedOracleIndex.calls.append(("where", n, where, column, zero))
        return self._scoped(q, n, where_mask({c: self._st[2][c] for c in range(COLUMNS)}, where, self.n), column, zero)

    def search_collapsed_within(self, q, n, rows, column, zero="single"):
        q = self._query(q, n)
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        ScopedOracleIndex.calls.append(("within", n, rows.tolist(), column, zero))
        in_scope = np.zeros(self.n, dtype=bool)
        in_scope[rows - self.row_offset] = True
        return self._scoped(q, n, in_scope, column, zero)


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_roots=8, d=16, seed=41):
    """The three-level KB of test_collapse_host.py: n_roots roots (level 0), 3 children each (level 1), 2
    grandchildren per child (level 2); the last root has no child.  {doc id: (parent id or None, level)}."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=ScopedOracleIndex)
    tree, i = {}, 0
    with kb.bulk_add_docs() as add_doc:
        for r in range(n_roots):
            root = add_doc(f"doc {i}"); tree[root] = (None, 0); i += 1
            for _ in range(3 if r < n_roots - 1 else 0):
                child = add_doc(f"doc {i}", parent_id=root); tree[child] = (root, 1); i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); tree[leaf] = (child, 2); i += 1
    return kb, ef, table, tree


def _expected(kb, table, query, n, levels):
    """Brute force over the docs' own vectors: among the docs of ``levels`` every parent is represented by its child
    with the highest (score, embedding id), a doc without a parent by itself; [(score, doc id)] of the n best."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text, parent_id, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    m = np.array([table[t] for _, _, t, _, _ in rows], dtype=np.float32)
    s = np.dot(m, np.array(table[query], dtype=np.float32))
    best = {}
    for i, (_, doc, _, par, level) in enumerate(rows):
        if level not in levels:
            continue
        g = ("doc", doc) if par is None else ("parent", par)
        best[g] = max(best.get(g, (-np.inf, -1)), (s[i], i))
    top = sorted(best.values(), reverse=True)[:max(n, 0)]
    return [(float(sc), rows[i][1]) for sc, i in top]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_levels_keep_the_collapse_inside_one_level(tmp_path, caplog):
    kb, ef, table, tree = _kb(tmp_path, "a.sqlite")
    per_level = {lv: sum(1 for _, l in tree.values() if l == lv) for lv in (0, 1, 2)}
    assert per_level == {0: 8, 1: 21, 2: 42}
    ScopedOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_collapsed("q 0", 5, levels=2)
    assert _got(got) == _expected(kb, table, "q 0", 5, {2}) and len(got) == 5
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 5 documents with query string: q 0", "got embedding for query!",
                     "computed 42 cosine similarities", "retrieved top 5 documents"]
    assert ScopedOracleIndex.calls == [("where", 5, [(0, "in", [3])], kb_mod.PARENT_COLUMN, "single")]
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])      # retrieve's shape
    # at most one document per level-1 parent, none from another level: 21 groups, whatever n
    for q, n in (("q 1", 1), ("q 1", 12), ("q 2", 21), ("q 2", 500), ("q 3", 0), ("q 3", -2)):
        got = kb.retrieve_collapsed(q, n, levels=2)
        assert _got(got) == _expected(kb, table, q, n, {2}) and len(got) == min(max(n, 0), 21), (q, n)
        assert all(r["doc"]["level"] == 2 and tree[r["doc"]["parent_id"]][1] == 1 for r in got)
        parents = [r["doc"]["parent_id"] for r in got]
        assert len(set(parents)) == len(parents)
        assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)
    # without levels one subtree can take several places; inside level 2 it takes one
    unscoped = kb.retrieve_collapsed("q 1", 36)
    assert {r["doc"]["level"] for r in unscoped} == {0, 1, 2}
    # level 1: one document per root that has children; level 0: the roots stand for themselves; several levels; an
    # iterable; a level nobody has
    assert len(kb.retrieve_collapsed("q 4", 500, levels=1)) == 7
    assert len(kb.retrieve_collapsed("q 4", 500, levels=0)) == 8
    for levels, groups in (((1, 2), 7 + 21), ([0, 2], 8 + 21), (range(3), 36), (np.int64(2), 21)):
        got = kb.retrieve_collapsed("q 5", 500, levels=levels)
        want = {int(lv) for lv in (levels if hasattr(levels, "__iter__") else [levels])}
        assert _got(got) == _expected(kb, table, "q 5", 500, want) and len(got) == groups, levels
    assert _got(kb.retrieve_collapsed("q 5", 500, levels=range(3))) == _got(kb.retrieve_collapsed("q 5", 500))   # every level: every doc
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        caplog.clear()
        assert kb.retrieve_collapsed("q 5", 4, levels=7) == []
    assert [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"][2] == "computed 0 cosine similarities"
    for bad in (-1, 1.5, "2", [0, None], True):
        with pytest.raises(ValueError):
            kb.retrieve_collapsed("q 5", 4, levels=bad)
    # a representative that is deleted hands over to the runner-up on its level
    best = kb.retrieve_collapsed("q 6", 1, levels=2)[0]["doc"]
    with kb.bulk_del_docs() as del_doc:
        del_doc(best["id"])
    after = kb.retrieve_collapsed("q 6", 21, levels=2)
    assert best["id"] not in {r["doc"]["id"] for r in after} and best["parent_id"] in {r["doc"]["parent_id"] for r in after}
    assert [d for _, d in _got(after)] == [d for _, d in _expected(kb, table, "q 6", 21, {2})]
    kb.close()
    assert OracleIndex.live == 0


def test_levels_none_is_the_unscoped_call(tmp_path, caplog):
    kb, ef, table, tree = _kb(tmp_path, "n.sqlite")
    ScopedOracleIndex.calls.clear()
    ColumnOracleIndex.set_calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        a = kb.retrieve_collapsed("q 0", 6)
        b = kb.retrieve_collapsed("q 0", 6, None)
        c = kb.retrieve_collapsed("q 0", 6, levels=None)
    assert _got(a) == _got(b) == _got(c)
    assert ScopedOracleIndex.calls == [("collapsed", 6, None, kb_mod.PARENT_COLUMN, "single")] * 3
    assert ColumnOracleIndex.set_calls == [(kb_mod.PARENT_COLUMN, 0, len(tree))]          # the level column is not installed
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 6 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(tree)} cosine similarities", "retrieved top 6 documents"] * 3
    kb.close()


def test_the_level_and_parent_columns_are_installed_once(tmp_path):
    kb, ef, table, tree = _kb(tmp_path, "c.sqlite")
    calls = ColumnOracleIndex.set_calls
    calls.clear()
    n = len(tree)
    kb.retrieve("q 0", 3)
    assert calls == []
    kb.retrieve_collapsed("q 0", 3, levels=2)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, n), (0, 0, n)]    # the parent column, then the level column: as retrieve_under
    kb.retrieve_collapsed("q 1", 3, levels=[1, 2])
    kb.retrieve_collapsed("q 1", 3)
    kb.retrieve_under("q 1", 3, next(d for d, (p, _) in tree.items() if p is None), levels=1)
    kb.retrieve_at_level("q 1", 3, 2)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, n), (0, 0, n)]
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, parent_id, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    st = kb.embeddings_matrix.index._st[2]
    assert st[kb_mod.PARENT_COLUMN].tolist() == [0 if p is None else p + 1 for _, p, _ in by_emb]
    assert st[0].tolist() == [lv + 1 for _, _, lv in by_emb]
    # bulk_add_docs passes both columns' values of the rows it appends: nothing is re-installed
    child = next(d for d, (p, lv) in tree.items() if lv == 1)
    table["late"] = table["q 5"]
    with kb.bulk_add_docs() as add_doc:
        late = add_doc("late", parent_id=child)
    assert kb.retrieve_collapsed("q 5", 1, levels=2)[0]["doc"]["id"] == late
    assert sorted(calls[2:]) == [(0, n, 1), (kb_mod.PARENT_COLUMN, n, 1)]
    kb.close()
    assert OracleIndex.live == 0


def test_async_retrieve_collapsed_with_levels_equals_sync(tmp_path, caplog):
    kb, ef, table, tree = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    asks = [("q 0", 5, 2), ("q 1", 1, 1), ("q 2", 36, (1, 2)), ("q 3", 500, 2), ("q 4", 0, 2), ("q 5", 9, None), ("q 6", 4, 9)]
    want = [_got(kb.retrieve_collapsed(*a)) for a in asks]
    assert [len(w) for w in want] == [5, 1, 28, 21, 0, 9, 0]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=ScopedOracleIndex)
        ColumnOracleIndex.set_calls.clear()
        ScopedOracleIndex.calls.clear()
        got = await asyncio.gather(*[akb.retrieve_collapsed(q, n, levels=lv) for q, n, lv in asks])
        # seven concurrent tasks, one installation of each column
        assert sorted(ColumnOracleIndex.set_calls) == [(0, 0, len(tree)), (kb_mod.PARENT_COLUMN, 0, len(tree))]
        assert sorted(c[0] for c in ScopedOracleIndex.calls) == ["collapsed"] + ["where"] * 6
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_collapsed("q 1", 9, levels=1)
            await akb.retrieve_collapsed("q 1", 9)
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 9 documents with query string: q 1", "got embedding for query!",
                     "computed 21 cosine similarities", "retrieved top 9 documents",
                     "retrieving 9 documents with query string: q 1", "got embedding for query!",
                     f"computed {len(tree)} cosine similarities", "retrieved top 9 documents"]
    assert OracleIndex.live == 0


class NoHandle:
    """What DeviceIndex's scoped collapsed searches touch before their argument checks are over: the handle raises."""

    _search_batch_collapsed_scoped = index_mod.DeviceIndex._search_batch_collapsed_scoped

    @staticmethod
    def _queries_2d(q):
        return np.ascontiguousarray(q, dtype=np.float32)

    def _pinned_handle(self):
        raise AssertionError("the handle was touched before the arguments were checked")

    @property
    def _lib(self):
        raise AssertionError("the library was touched before the arguments were checked")


def test_arguments_are_checked_before_the_handle_is_touched():
    q = np.zeros((1, 4), dtype=np.float32)
    where_call = index_mod.DeviceIndex.search_batch_collapsed_where
    within_call = index_mod.DeviceIndex.search_batch_collapsed_within
    for bad in (-1, 4, True, 1.0, "1", None):                     # the column
        with pytest.raises(ValueError):
            where_call(NoHandle(), q, 3, [(0, "in", [1])], bad)
        with pytest.raises(ValueError):
            within_call(NoHandle(), q, 3, [0, 1], bad)
    for bad in ("", "both", None, 1):                             # the zero mode
        with pytest.raises(ValueError):
            where_call(NoHandle(), q, 3, [(0, "in", [1])], 1, bad)
        with pytest.raises(ValueError):
            within_call(NoHandle(), q, 3, [0, 1], 1, bad)
    for bad in ([(4, "in", [1])], [(0, "between", (1, 2))], [(0, "in", [-1])], [(0, "range", (1,))], [(0, "in")],
                [(0, "in", [1])] * 5):                            # the terms
        with pytest.raises((ValueError, NotImplementedError)):
            where_call(NoHandle(), q, 3, bad, 1)
    with pytest.raises(ValueError):                               # a 2-D query to the single-query forms
        index_mod.DeviceIndex.search_collapsed_where(NoHandle(), q, 3, [(0, "in", [1])], 1)
    with pytest.raises(ValueError):
        index_mod.DeviceIndex.search_collapsed_within(NoHandle(), q, 3, [0, 1], 1)
    # well-formed arguments do reach the handle
    with pytest.raises(AssertionError, match="before the arguments were checked"):
        where_call(NoHandle(), q, 3, [(0, "in", [1])], 1)
    with pytest.raises(AssertionError, match="before the arguments were checked"):
        within_call(NoHandle(), q, 3, [0, 1], 1, "group")


def test_the_header_declares_both_entries():
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "svs_amd.h")).read(), flags=re.S))
    assert ("int32_t svs_index_search_collapsed_where(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, "
            "const svs_where_term_t* terms, int32_t nterms, int32_t column, int32_t zero_mode, float* out_scores, int64_t* out_rows, "
            "uint32_t* out_values , int32_t* out_counts , int64_t* out_groups , int64_t* out_matched );") in hdr
    assert ("int32_t svs_index_search_collapsed_rows(svs_index* idx, const float* queries, int32_t nq, int32_t d, int32_t k, "
            "const int64_t* rows, int64_t nrows, int32_t column, int32_t zero_mode, float* out_scores, int64_t* out_rows, "
            "uint32_t* out_values, int32_t* out_counts, int64_t* out_groups, int64_t* out_matched);") in hdr
    for name in ("svs_index_search_collapsed_where", "svs_index_search_collapsed_rows"):
        assert len(_native.SIGNATURES[name][1]) == 15
    assert "svs_internal_collapse_scope_kernel_ms" in _native.INTERNAL
    assert "svs_internal_collapse_scope_kernel_ms" in open(os.path.join(ROOT, "svs_amd", "csrc", "internal.h")).read()


def test_matrix_ops_map_embedding_ids():
    from svs_amd.matrix import _Lookup, collapsed_where_op, collapsed_within_op
    m = _unit(np.random.default_rng(2), 30, 8)
    idx = ScopedOracleIndex(m, 0, 100)
    idx.set_column(2, np.arange(30) // 4, 100)                   # rows 0 .. 3 carry 0, then groups of four
    idx.set_column(0, np.arange(30) % 2, 100)                    # the odd rows are the scope
    arr = np.arange(30, dtype=np.int64) * 7 + 5                  # row r holds embedding id 7 r + 5
    for zero, groups in (("single", 2 + 7), ("group", 8)):
        native, finish = collapsed_where_op(m[9], 6, [(0, "in", [1])], 2, zero)
        used, (hits, g, matched) = native(idx, None)
        assert used is idx and len(hits) == 6 and (g, matched) == (groups, 15)
        assert all(100 <= r < 130 and (r - 100) % 2 == 1 for _, r, _ in hits)
        out, og, om = finish((used, (hits, g, matched)), arr)
        assert (og, om) == (groups, 15) and out == [(s, 7 * (r - 100) + 5, v) for s, r, v in hits]
        assert out[0][1] == 7 * 9 + 5 and out[0][2] == 9 // 4 and all(isinstance(x, int) for o in out for x in o[1:])
        # the same scope as a list of embedding ids: ids -> rows going in, rows -> ids coming out
        ids = arr[1::2][::-1]
        native, finish = collapsed_within_op(m[9], 6, ids, 2, zero)
        ScopedOracleIndex.calls.clear()
        res = native(idx, _Lookup(arr))
        assert ScopedOracleIndex.calls == [("within", 6, (np.arange(1, 30, 2)[::-1] + 100).tolist(), 2, zero)]
        assert finish(res, arr) == (out, groups, 15)
    with pytest.raises(KeyError):
        collapsed_within_op(m[9], 6, [5, 6], 2)[0](idx, _Lookup(arr))      # 6 is no embedding id of the matrix
    idx.release()


def test_multi_and_sharded_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[ScopedOracleIndex(m[:20], 0, 0), ScopedOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    from svs_amd.sharded import ShardedIndex
    for name, scope in (("search_collapsed_where", [(0, "in", [1])]), ("search_batch_collapsed_where", [(0, "in", [1])]),
                        ("search_collapsed_within", [0, 1]), ("search_batch_collapsed_within", [0, 1])):
        q = m[:2] if "batch" in name else m[0]
        with pytest.raises(NotImplementedError):
            getattr(mi, name)(q, 3, scope, 1)
        with pytest.raises(NotImplementedError):
            getattr(ShardedIndex, name)(None, q, 3, scope, 1)
    mi.release()


def test_scoped_kernels_exist_once_and_use_no_scratch():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    names = _demangle([n for n in table if "scoped_" in n])
    for kernel in ("scoped_write_kernel", "scoped_values_kernel"):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == 1, (kernel, sorted(names.values()))
        r = table[hits[0]]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{kernel}: {r}"
    assert len(names) == 2, sorted(names.values())

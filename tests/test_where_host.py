"""CPU: predicate search above the kernel -- the checking and packing of a ``where`` list (svs_amd.index), the parent
values of ``KB.retrieve_under`` and their errors, ``retrieve_under`` / ``AsyncKB.retrieve_under`` against
``retrieve_within`` and the per-column bookkeeping of ``DeviceEmbeddingsMatrix`` through a numpy double of DeviceIndex
(tests/where_backend.py), the multi-device refusals, and the new kernels' resource report."""
import asyncio
import ctypes as C
import logging
import os

import numpy as np
import pytest

from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources
from where_backend import ColumnOracleIndex

import svs_amd
from svs_amd import _native, index as index_mod, kb as kb_mod, multi as multi_mod
from svs_amd.kb import embedding_to_bytes


# ---- the where list ----------------------------------------------------------------------------------------------
def test_where_terms_are_normalised():
    got = index_mod.where_terms([(0, "in", [7, 1, 7]), (1, "not in", np.array([5], dtype=np.int64)), (2, "range", (3, 9)),
                                 (3, "no_bits", 0x80000000)])
    assert [(c, op, neg, a, b) for c, op, neg, a, b, _ in got] == [
        (0, _native.WHERE_IN, 0, 0, 0), (1, _native.WHERE_IN, 1, 0, 0), (2, _native.WHERE_RANGE, 0, 3, 9),
        (3, _native.WHERE_ANY_BITS, 1, 0x80000000, 0)]
    assert got[0][5].tolist() == [7, 1, 7] and got[0][5].dtype == np.uint32 and got[1][5].tolist() == [5]   # (the library sorts)
    assert got[2][5] is None and got[3][5] is None
    for op, (code, neg) in index_mod.WHERE_OPS.items():
        arg = [1] if "in" == op.split()[-1] else (1, 2) if "range" in op else 3
        (c, gc, gn, *_), = index_mod.where_terms([(np.int64(2), op, arg)])
        assert (c, gc, gn) == (2, code, neg)
    assert sorted(index_mod.WHERE_OPS) == sorted(["in", "not in", "range", "not range", "any_bits", "no_bits", "all_bits", "not all_bits"])
    assert index_mod.where_terms([]) == [] and index_mod.where_terms([(0, "in", [])])[0][5].tolist() == []
    assert index_mod.where_terms([(0, "range", (0xFFFFFFFF, 0)), (0, "all_bits", 0xFFFFFFFF)])[0][3:5] == (0xFFFFFFFF, 0)
    assert index_mod.where_terms([(1, "in", range(3)), (1, "in", (x for x in (9, 9)))])[1][5].tolist() == [9, 9]


@pytest.mark.parametrize("bad", [
    [(0, "like", 1)], [(0, None, 1)], [(4, "in", [1])], [(-1, "in", [1])], [(True, "in", [1])], [(1.0, "in", [1])],
    [(0, "in", [-1])], [(0, "in", [1 << 32])], [(0, "in", [True])], [(0, "in", [1.5])], [(0, "in", 3)], [(0, "in", "12")],
    [(0, "range", (1,))], [(0, "range", 3)], [(0, "range", (-1, 2))], [(0, "range", (0, 1 << 32))], [(0, "range", (0, True))],
    [(0, "range", (0.0, 1))], [(0, "any_bits", -1)], [(0, "all_bits", 1 << 32)], [(0, "no_bits", False)], [(0, "any_bits", 1.0)],
    [(0, "any_bits", [1])], [(0, "in")], [7], [(0, "in", [1])] * 5,
    [(0, "in", range(1025))], [(0, "in", range(600)), (1, "not in", range(425))],
])
def test_bad_where_lists_raise_before_the_call(bad):
    with pytest.raises(ValueError):
        index_mod.where_terms(bad)
    with pytest.raises(ValueError):
        index_mod.pack_where(bad)


def test_limits_are_on_distinct_members():
    assert len(index_mod.where_terms([(0, "in", range(1024))])) == 1
    assert len(index_mod.where_terms([(0, "in", list(range(512)) * 3), (1, "not in", range(512))])) == 2
    assert len(index_mod.where_terms([(0, "range", (0, 1))] * 4)) == 4


def test_terms_are_packed_as_the_header_lays_them_out():
    arr, n, keep = index_mod.pack_where([(3, "not in", [9, 2, 9]), (1, "range", (4, 0xFFFFFFFF)), (0, "all_bits", 6), (2, "in", [])])
    assert n == 4 and len(arr) == 4
    t = arr[0]
    assert (t.column, t.op, t.negate, t.nset) == (3, 0, 1, 3)
    assert np.ctypeslib.as_array(C.cast(t.set, C.POINTER(C.c_uint32)), (3,)).tolist() == [9, 2, 9]
    assert (arr[1].column, arr[1].op, arr[1].negate, arr[1].a, arr[1].b) == (1, 1, 0, 4, 0xFFFFFFFF)
    assert (arr[2].column, arr[2].op, arr[2].negate, arr[2].a) == (0, 3, 0, 6)
    assert (arr[3].column, arr[3].op, arr[3].nset, arr[3].set) == (2, 0, 0, None)
    assert index_mod.pack_where([]) == (None, 0, [])
    # svs_where_term_t: three i32, two u32, a pointer on its own 8-byte boundary, one i32, padded to 8
    f = _native.WhereTerm
    assert [getattr(f, name).offset for name, _ in f._fields_] == [0, 4, 8, 12, 16, 24, 32] and C.sizeof(f) == 40
    assert (_native.COLUMNS_MAX, _native.WHERE_MAX_TERMS) == (4, 4)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svs_amd.h")).read()
    assert "#define SVS_COLUMNS_MAX 4" in hdr and "#define SVS_WHERE_MAX_TERMS 4" in hdr
    assert "SVS_WHERE_IN = 0, SVS_WHERE_RANGE = 1, SVS_WHERE_ANY_BITS = 2, SVS_WHERE_ALL_BITS = 3" in hdr


def test_column_numbers_are_checked_before_the_call():
    for bad in (-1, 4, True, 1.0, "1", None):
        with pytest.raises(ValueError):
            index_mod.column_index(bad)
        with pytest.raises(ValueError):
            index_mod.DeviceIndex.set_column(None, bad, [1])
        with pytest.raises(ValueError):
            index_mod.DeviceIndex.column(None, bad)
    assert [index_mod.column_index(c) for c in (0, np.int32(3))] == [0, 3]


# ---- the KB's parent values --------------------------------------------------------------------------------------
def test_parent_values_and_their_errors():
    assert kb_mod.PARENT_COLUMN == 1
    assert kb_mod._parent_value(None) == 0 and kb_mod._parent_value(0) == 1 and kb_mod._parent_value(np.int64(41)) == 42
    assert kb_mod._parent_value(0xFFFFFFFE) == 0xFFFFFFFF
    for bad in (0xFFFFFFFF, 1 << 40, -1, True, 1.0, "3"):
        with pytest.raises(ValueError):
            kb_mod._parent_value(bad)
    assert kb_mod._parent_values(5) == [6] and kb_mod._parent_values([9, 2, 9, np.int32(2)]) == [3, 10]
    assert kb_mod._parent_values([]) == [] and kb_mod._parent_values(range(1024)) == list(range(1, 1025))
    for bad in (range(1025), [1, None], None, "12", 2.0, [0xFFFFFFFF], [-3], True, [False]):
        with pytest.raises(ValueError):
            kb_mod._parent_values(bad)
    assert kb_mod._parent_column([None, 0, 7]) == [0, 1, 8] and kb_mod._parent_column([1, 0xFFFFFFFF]) is None
    assert kb_mod._under_where([4, 3], None) == [(1, "in", [4, 5])]
    assert kb_mod._under_where(3, (1, 0)) == [(1, "in", [4]), (0, "in", [1, 2])]
    with pytest.raises(ValueError):
        kb_mod._under_where(3, -1)


# ---- retrieve_under on the double --------------------------------------------------------------------------------
def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_roots=8, d=16, seed=33):
    """A three-level KB: n_roots roots, 3 children each, 2 grandchildren per child; the last root has no child.
    ({doc id: parent id or None}, {doc id: level})."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=ColumnOracleIndex)
    parent, level, i = {}, {}, 0
    with kb.bulk_add_docs() as add_doc:
        for r in range(n_roots):
            root = add_doc(f"doc {i}"); parent[root], level[root] = None, 0; i += 1
            for _ in range(3 if r < n_roots - 1 else 0):
                child = add_doc(f"doc {i}", parent_id=root); parent[child], level[child] = root, 1; i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); parent[leaf], level[leaf] = child, 2; i += 1
    return kb, ef, table, parent, level


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _children(parent, level, parents, levels=None):
    return [d for d, p in parent.items() if p in parents and (levels is None or level[d] in levels)]


def test_retrieve_under_equals_retrieve_within_over_the_children(tmp_path, caplog):
    kb, ef, table, parent, level = _kb(tmp_path, "u.sqlite")
    roots = [d for d, lv in level.items() if lv == 0]
    mids = [d for d, lv in level.items() if lv == 1]
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_under("q 0", 2, roots[0])
    assert _got(got) == _got(kb.retrieve_within("q 0", 2, _children(parent, level, {roots[0]}))) and len(got) == 2
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines[:4] == ["retrieving 2 documents with query string: q 0", "got embedding for query!",
                         "computed 3 cosine similarities", "retrieved top 2 documents"]
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])
    asks = [(roots[0], None), (roots[:3], None), ([roots[1], mids[0], mids[5]], None), (roots[-1], None), (range(10000, 10003), None),
            ([roots[0], mids[0]], 2), ([roots[0], mids[0]], (1,)), (roots + mids, (0,)), (roots + mids, (1, 2)), ([], None), ([], 1),
            (np.int64(mids[2]), [2, 2])]
    for parents, levels in asks:
        ps = {int(parents)} if isinstance(parents, (int, np.integer)) else set(parents)
        ls = None if levels is None else {levels} if isinstance(levels, int) else set(levels)
        ids = _children(parent, level, ps, ls)
        got = kb.retrieve_under("q 1", 500, parents, levels)
        assert _got(got) == _got(kb.retrieve_within("q 1", 500, ids)) and len(got) == len(ids), (parents, levels)
        assert all(r["doc"]["parent_id"] in ps for r in got)
    assert kb.retrieve_under("q 1", 5, roots[-1]) == [] and kb.retrieve_under("q 1", 5, []) == []
    assert kb.retrieve_under("q 1", 0, roots[0]) == []
    # the stored value is parent_id + 1 (0: no parent) in column 1, the level + 1 in column 0, in embedding-id order
    with kb.db.transaction():
        by_emb = sorted(kb.db.conn.execute("SELECT embedding, parent_id, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    st = kb.embeddings_matrix.index._st[2]
    assert st[1].tolist() == [0 if p is None else p + 1 for _, p, _ in by_emb] and st[0].tolist() == [lv + 1 for _, _, lv in by_emb]
    assert not st[2:].any()
    for bad in (-1, [0, -2], 1.0, [True], "1", range(1025), [0xFFFFFFFF], None):
        with pytest.raises(ValueError):
            kb.retrieve_under("q 0", 3, bad)
    with pytest.raises(ValueError):
        kb.retrieve_under("q 0", 3, roots[0], levels=-1)
    kb.close()
    assert OracleIndex.live == 0


def test_the_parent_column_is_installed_once_per_generation_and_follows_appends(tmp_path):
    kb, ef, table, parent, level = _kb(tmp_path, "g.sqlite")
    calls = ColumnOracleIndex.set_calls
    calls.clear()
    kb.load()
    kb.retrieve("q 0", 3)
    kb.retrieve_at_level("q 0", 3, 1)
    n = len(level)
    assert calls == [(0, 0, n)]                                   # the level column alone: column 1 is installed lazily
    root = next(d for d, lv in level.items() if lv == 0)
    child = next(d for d, lv in level.items() if lv == 1)
    kb.retrieve_under("q 0", 3, root)
    assert calls == [(0, 0, n), (1, 0, n)]                        # one call, the whole range
    kb.retrieve_under("q 2", 3, [root, child], levels=2)
    assert calls == [(0, 0, n), (1, 0, n)]
    first = kb.embeddings_matrix.index
    # bulk_add_docs with both columns installed: the new rows' values go in behind the append, nothing is re-installed
    table["late root"], table["late leaf"] = table["q 3"], table["q 4"]
    with kb.bulk_add_docs() as add_doc:
        a = add_doc("late root")
        b = add_doc("late leaf", parent_id=child)
        add_doc("doc 399", parent_id=root, no_embedding=True)
    parent[a], level[a], parent[b], level[b] = None, 0, child, 2
    assert kb.embeddings_matrix.index is first and sorted(calls[2:]) == [(0, n, 2), (1, n, 2)]
    assert first._st[2][1, n:].tolist() == [0, child + 1] and first._st[2][0, n:].tolist() == [1, 3]
    assert [r["doc"]["id"] for r in kb.retrieve_under("q 4", 1, child)] == [b]
    assert _got(kb.retrieve_under("q 4", 500, child)) == _got(kb.retrieve_within("q 4", 500, _children(parent, level, {child})))
    assert len(calls) == 4
    # deletions: the tombstoned rows drop out
    gone = _children(parent, level, {child})[0]                   # (an early row: the newest embedding id stays the largest)
    with kb.bulk_del_docs() as del_doc:
        del_doc(gone)
    del parent[gone], level[gone]
    assert len(kb.retrieve_under("q 4", 500, child)) == 2
    assert _got(kb.retrieve_under("q 4", 500, child)) == _got(kb.retrieve_within("q 4", 500, _children(parent, level, {child})))
    # an append WITHOUT values: both columns count as not installed; each retrieval installs what it names, once
    table["bare"] = table["q 5"]
    with kb.db.transaction():
        doc, lv = kb.db.add_doc_at("bare", child, None)
        emb = kb.db.set_doc_embedding(doc, embedding_to_bytes(table["bare"]))
    assert kb.embeddings_matrix.append(np.array([table["bare"]], dtype=np.float32), [emb])
    assert first._st[2][1, -1] == 0 and len(calls) == 4
    assert [r["doc"]["id"] for r in kb.retrieve_under("q 5", 1, child)] == [doc]
    assert calls[4:] == [(1, 0, n + 3)] and first._st[2][1, -1] == child + 1 and first._st[2][0, -1] == 0
    assert [r["doc"]["id"] for r in kb.retrieve_under("q 5", 1, child, levels=2)] == [doc]
    assert calls[5:] == [(0, 0, n + 3)] and first._st[2][0, -1] == 3
    # labels alone with the append: the level column stays installed, the parent column does not
    table["half"] = table["q 6"]
    with kb.db.transaction():
        doc2, _ = kb.db.add_doc_at("half", child, None)
        emb2 = kb.db.set_doc_embedding(doc2, embedding_to_bytes(table["half"]))
    assert kb.embeddings_matrix.append(np.array([table["half"]], dtype=np.float32), [emb2], labels=[3])
    assert calls[6:] == [(0, n + 3, 1)]
    assert [r["doc"]["id"] for r in kb.retrieve_under("q 6", 1, child, levels=2)] == [doc2]
    assert calls[7:] == [(1, 0, n + 4)]
    # a stored parent id that does not fit: the append leaves the column not installed and the next retrieval raises
    table["far"] = table["q 7"]
    with kb.db.transaction():
        kb.db.conn.execute("INSERT INTO docs (id, parent_id, level, text, embedding, meta) VALUES (?, NULL, 0, 'big', NULL, NULL)", (0xFFFFFFFF,))
        doc3, _ = kb.db.add_doc_at("far", 0xFFFFFFFF, None)
        emb3 = kb.db.set_doc_embedding(doc3, embedding_to_bytes(table["far"]))
    assert kb.embeddings_matrix.append(np.array([table["far"]], dtype=np.float32), [emb3], labels=[2],
                                       columns={kb_mod.PARENT_COLUMN: kb_mod._parent_column([0xFFFFFFFF])})
    with pytest.raises(ValueError):
        kb.retrieve_under("q 7", 1, child)
    assert len(kb.retrieve_at_level("q 7", 1, 1)) == 1            # (the level column is not affected)
    kb.close()
    assert OracleIndex.live == 0


def test_async_retrieve_under_equals_sync(tmp_path, caplog):
    kb, ef, table, parent, level = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    roots = [d for d, lv in level.items() if lv == 0]
    mids = [d for d, lv in level.items() if lv == 1]
    asks = [("q 0", 5, roots[0]), ("q 1", 9, roots[:4]), ("q 2", 500, roots + mids, 2), ("q 3", 4, [mids[0], roots[2]], (1, 2)),
            ("q 4", 3, roots[-1]), ("q 5", 3, [])]
    want = [_got(kb.retrieve_under(*a)) for a in asks]
    assert [len(w) for w in want] == [3, 9, 42, 4, 0, 0]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=ColumnOracleIndex)
        ColumnOracleIndex.set_calls.clear()
        got = await asyncio.gather(*[akb.retrieve_under(*a) for a in asks])
        assert sorted(ColumnOracleIndex.set_calls) == [(0, 0, len(level)), (1, 0, len(level))]   # six tasks, one installation each
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_under("q 1", 9, roots[:4])
        async with akb.bulk_add_docs() as add_doc:
            table["late"] = table["q 6"]
            new = await add_doc("late", parent_id=roots[-1])
        late = await akb.retrieve_under("q 6", 1, roots[-1])
        assert [r["doc"]["id"] for r in late] == [new]
        assert sorted(ColumnOracleIndex.set_calls[2:]) == [(0, len(level), 1), (1, len(level), 1)]
        with pytest.raises(ValueError):
            await akb.retrieve_under("q 0", 3, range(1025))
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 9 documents with query string: q 1", "got embedding for query!",
                     "computed 12 cosine similarities", "retrieved top 9 documents"]
    assert OracleIndex.live == 0


def test_multi_and_sharded_column_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[ColumnOracleIndex(m[:20], 0, 0), ColumnOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    for call in (lambda: mi.search_where(m[0], 3, [(1, "in", [1])]), lambda: mi.search_batch_where(m[:2], 3, []),
                 lambda: mi.count_where([]), lambda: mi.set_column(1, np.ones(40, dtype=np.uint32)), lambda: mi.column(1)):
        with pytest.raises(NotImplementedError):
            call()
    mi.release()
    from svs_amd.sharded import ShardedIndex
    for call in (lambda: ShardedIndex.search_where(None, m[0], 3, []), lambda: ShardedIndex.search_batch_where(None, m[:2], 3, []),
                 lambda: ShardedIndex.count_where(None, []), lambda: ShardedIndex.set_column(None, 1, [1]),
                 lambda: ShardedIndex.column(None, 1)):
        with pytest.raises(NotImplementedError):
            call()


def test_where_kernels_use_no_scratch():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    names = _demangle([n for n in table if "where_" in n])
    for kernel in ("where_count_kernel", "where_write_kernel"):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == 1, (kernel, sorted(names.values()))
        r = table[hits[0]]
        # (the terms, the column pointers and eight ballots are all scalar registers: a few of them are parked in
        #  VGPR lanes, which is not memory -- scratch and VGPR spills are what must stay 0)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{kernel}: {r}"

"""CPU: group-combined retrieval above the kernel -- parent <-> column value, emb id <-> row <-> doc mapping of
``KB.retrieve_collapsed_combined`` / ``AsyncKB.retrieve_collapsed_combined`` through a numpy double of DeviceIndex whose
``search_collapsed_combined`` is the numpy model of the definition (collapsed_combined_model.py) over oracle scores; the
argument checks; the multi-device refusals; ``collapsed_combined_op``; and the new kernels' resource report."""
import asyncio
import logging
import os
import re

import numpy as np
import pytest

import combine_model
from collapsed_combined_model import collapsed_combined
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources
from where_backend import ColumnOracleIndex

import svs_amd
from svs_amd import _native, index as index_mod, kb as kb_mod, multi as multi_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class GroupCombineOracleIndex(ColumnOracleIndex):
    """ColumnOracleIndex whose ``search_collapsed_combined`` is the model over its own state."""

    calls = []          # (m, n, column, op, weights or None, zero) of every call, all instances

    def share(self):
        self._check()
        return GroupCombineOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_collapsed_combined(self, vectors, n, column, op="max", weights=None, zero="single"):
        self._check()
        assert isinstance(n, int)
        v = np.asarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.d or not 1 <= v.shape[0] <= index_mod.COMBINE_MAX_VECTORS or op not in index_mod.COMBINE_OPS:
            raise ValueError("bad combined query")
        w = None if weights is None else np.asarray(weights, dtype=np.float32)
        if w is not None and (w.shape != (v.shape[0],) or not np.isfinite(w).all()):
            raise ValueError("bad weights")
        GroupCombineOracleIndex.calls.append((v.shape[0], n, column, op, None if w is None else w.tolist(), zero))
        single = index_mod.collapse_zero_mode(zero) == _native.COLLAPSE_ZERO_SINGLE
        s, r, val, groups = collapsed_combined([self.scores(x) for x in v], w, op, self._st[2][column], self._st[1], single, n)
        return list(zip(s.astype(np.float64).tolist(), (r + self.row_offset).tolist(), val.tolist())), groups


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_roots=8, d=16, seed=43):
    """n_roots roots, 3 children each, 2 grandchildren per child; the last root has no child.  {doc id: parent id or None}."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}
    embed_calls = []

    async def ef(ts):
        embed_calls.append(list(ts))
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=GroupCombineOracleIndex)
    parent, i = {}, 0
    with kb.bulk_add_docs() as add_doc:
        for r in range(n_roots):
            root = add_doc(f"doc {i}"); parent[root] = None; i += 1
            for _ in range(3 if r < n_roots - 1 else 0):
                child = add_doc(f"doc {i}", parent_id=root); parent[child] = root; i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); parent[leaf] = child; i += 1
    embed_calls.clear()
    return kb, ef, table, parent, embed_calls


def _expected(kb, table, queries, n, op, weights):
    """The definition over the docs' own vectors by a loop over the parents: per parent and query the best child's
    score, combined by combine_model; the parent is represented by the child with the highest (row-level combined
    score, embedding id); a doc without a parent stands for itself.  [(score, doc id)] of the n best."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text, parent_id FROM docs WHERE embedding IS NOT NULL").fetchall())
    m = np.array([table[t] for _, _, t, _ in rows], dtype=np.float32)
    s = [np.dot(m, np.array(table[q], dtype=np.float32)) for q in queries]
    w = None if weights is None else np.asarray(weights, dtype=np.float32)
    c_row = combine_model.combine(s, w, op)
    members = {}
    for i, (_, doc, _, par) in enumerate(rows):
        members.setdefault(("doc", doc) if par is None else ("parent", par), []).append(i)
    ranked = []
    for rows_of in members.values():
        c = combine_model.combine([np.array([max(sj[i] for i in rows_of)], dtype=np.float32) for sj in s], w, op)[0]
        ranked.append((float(c), max((float(c_row[i]), i) for i in rows_of)[1]))
    ranked.sort(reverse=True)
    return [(sc, rows[i][1]) for sc, i in ranked[:max(n, 0)]]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_binding_and_header_agree():
    assert "svs_index_search_collapsed_combined" in _native.SIGNATURES
    assert {"svs_internal_multi_scores", "svs_internal_collapsed_combined_kernel_ms"} <= set(_native.INTERNAL)
    with open(os.path.join(ROOT, "include", "svs_amd.h")) as f:
        h = f.read()
    decl = re.search(r"int32_t svs_index_search_collapsed_combined\((.*?)\);", h, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 15
    assert len(_native.SIGNATURES["svs_index_search_collapsed_combined"][1]) == 15
    with open(os.path.join(ROOT, "svs_amd", "csrc", "internal.h")) as f:
        assert "svs_internal_multi_scores" in f.read() and "svs_internal_multi_scores" not in h


def test_retrieve_collapsed_combined_keeps_one_document_per_parent(tmp_path, caplog):
    kb, ef, table, parent, embed_calls = _kb(tmp_path, "a.sqlite")
    qs = ["q 0", "q 1", "q 2"]
    GroupCombineOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_collapsed_combined(qs, 5)
    assert embed_calls == [qs]                                                               # ONE embedding call
    assert GroupCombineOracleIndex.calls == [(3, 5, kb_mod.PARENT_COLUMN, "max", None, "single")]
    assert _got(got) == _expected(kb, table, qs, 5, "max", None) and len(got) == 5
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == [f"retrieving 5 documents with 3 query strings: {qs}", "got embeddings for the queries!",
                     f"computed {len(parent)} x 3 cosine similarities", "retrieved top 5 documents"]
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])        # retrieve's shape
    groups = 8 + 7 + 21                     # 8 roots stand for themselves, 7 roots and 21 children are parents
    w = [1.0, -0.5, 0.25]
    for mode, op in (("any", "max"), ("all", "min"), ("sum", "sum")):
        for weights in (None, w):
            for n in (1, 12, groups, 500, 0, -2):
                got = kb.retrieve_collapsed_combined(qs, n, mode=mode, weights=weights)
                assert _got(got) == _expected(kb, table, qs, n, op, weights), (mode, weights, n)
                assert len(got) == min(max(n, 0), groups)
                seen = [("doc", r["doc"]["id"]) if r["doc"]["parent_id"] is None else ("parent", r["doc"]["parent_id"]) for r in got]
                assert len(set(seen)) == len(seen)                                           # at most one per parent
                assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)
    # the case the entry exists for: one child of a parent IS query 4, another IS query 5 -- under "all" the parent scores
    # 1.0 against both and comes first, although no single document is close to both
    child = next(d for d, p in parent.items() if p is not None and parent[p] is None)
    table["facet a"], table["facet b"] = table["q 4"], table["q 5"]
    with kb.bulk_add_docs() as add_doc:
        twins = [add_doc("facet a", parent_id=child), add_doc("facet b", parent_id=child)]
    got = kb.retrieve_collapsed_combined(["q 4", "q 5"], 3, mode="all")
    assert _got(got) == _expected(kb, table, ["q 4", "q 5"], 3, "min", None)
    assert got[0]["doc"]["id"] in twins and got[0]["score"] == pytest.approx(1.0, abs=1e-6)
    vecs = np.array(list(table.values()), dtype=np.float32)
    a, b = (np.dot(vecs, np.array(table[q], dtype=np.float32)) for q in ("q 4", "q 5"))
    assert np.minimum(a, b).max() < 0.9                                                      # what a row-level "all" could see at best
    # deletions: the runner-up takes over as the representative, the parent keeps the facet that is left
    with kb.bulk_del_docs() as del_doc:
        del_doc(got[0]["doc"]["id"])
    left = kb.retrieve_collapsed_combined(["q 4", "q 5"], 3, mode="any")
    assert left[0]["doc"]["id"] in twins and left[0]["doc"]["id"] != got[0]["doc"]["id"]
    kb.close()
    assert OracleIndex.live == 0


def test_the_parent_column_is_installed_once(tmp_path):
    kb, ef, table, parent, _ = _kb(tmp_path, "g.sqlite")
    calls = ColumnOracleIndex.set_calls
    calls.clear()
    kb.retrieve("q 0", 3)
    assert calls == []                                           # lazily: nothing before the first retrieval that needs it
    kb.retrieve_collapsed_combined(["q 0", "q 1"], 3)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, len(parent))]     # through ensure_column, once, the whole range
    kb.retrieve_collapsed_combined(["q 2"], 3)
    assert calls == [(kb_mod.PARENT_COLUMN, 0, len(parent))]
    kb.close()
    assert OracleIndex.live == 0


def test_arguments_are_checked(tmp_path):
    kb, ef, table, parent, embed_calls = _kb(tmp_path, "e.sqlite", n_roots=2)
    GroupCombineOracleIndex.calls.clear()
    for bad in ([], [f"q {i % 8}" for i in range(9)]):
        with pytest.raises(ValueError):
            kb.retrieve_collapsed_combined(bad, 3)
    with pytest.raises(ValueError):
        kb.retrieve_collapsed_combined(["q 0"], 3, mode="best")
    for weights in ([1.0], [1.0, float("nan")], [1.0, float("inf")], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            kb.retrieve_collapsed_combined(["q 0", "q 1"], 3, mode="sum", weights=weights)
    assert embed_calls == [] and GroupCombineOracleIndex.calls == []      # refused before anything is embedded or searched
    kb.close()
    # DeviceIndex: shapes, op, weights, column and zero mode are checked before the handle is touched
    v = np.zeros((1, 2, 4), dtype=np.float32)
    batch = index_mod.DeviceIndex.search_batch_collapsed_combined
    for args in ((v[0], 3, 1), (np.zeros((1, 9, 4), dtype=np.float32), 3, 1), (np.zeros((1, 0, 4), dtype=np.float32), 3, 1),
                 (v, 3, 1, "avg"), (v, 3, 1, "sum", [1.0, 2.0]), (v, 3, 1, "sum", [[1.0]]),
                 (v, 3, -1), (v, 3, 4), (v, 3, True), (v, 3, "1"), (v, 3, 1, "max", None, "both")):
        with pytest.raises(ValueError):
            batch(None, *args)
    one = index_mod.DeviceIndex.search_collapsed_combined
    with pytest.raises(ValueError):
        one(None, v, 3, 1)                                                # a 3-D query
    with pytest.raises(ValueError):
        one(None, v[0], 3, 1, "sum", [[1.0, 2.0]])                        # 2-D weights


def test_async_retrieve_collapsed_combined_equals_sync(tmp_path, caplog):
    kb, ef, table, parent, _ = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    asks = [(["q 0", "q 1"], 5, "any", None), (["q 1"], 1, "all", None), (["q 2", "q 3", "q 4"], 36, "sum", [1.0, -1.0, 0.5]),
            (["q 3", "q 0"], 500, "all", [2.0, 0.5]), (["q 4", "q 5"], 0, "any", None), (["q 5", "q 6"], 9, "all", None)]
    want = [_got(kb.retrieve_collapsed_combined(q, n, mode=mode, weights=w)) for q, n, mode, w in asks]
    assert [len(x) for x in want] == [5, 1, 36, 36, 0, 9]
    ops = {"any": "max", "all": "min", "sum": "sum"}
    assert want == [_expected(kb, table, q, n, ops[mode], w) for q, n, mode, w in asks]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=GroupCombineOracleIndex)
        ColumnOracleIndex.set_calls.clear()
        got = await asyncio.gather(*[akb.retrieve_collapsed_combined(q, n, mode=mode, weights=w) for q, n, mode, w in asks])
        assert ColumnOracleIndex.set_calls == [(kb_mod.PARENT_COLUMN, 0, len(parent))]      # six concurrent tasks, one installation
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_collapsed_combined(["q 1", "q 2"], 9)
        with pytest.raises(ValueError):
            await akb.retrieve_collapsed_combined([], 3)
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 9 documents with 2 query strings: ['q 1', 'q 2']", "got embeddings for the queries!",
                     f"computed {len(parent)} x 2 cosine similarities", "retrieved top 9 documents"]
    assert OracleIndex.live == 0


def test_multi_and_sharded_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[GroupCombineOracleIndex(m[:20], 0, 0), GroupCombineOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError, match="per device"):
        mi.search_collapsed_combined(m[:2], 3, 1)
    with pytest.raises(NotImplementedError, match="per device"):
        mi.search_batch_collapsed_combined(m[None, :2], 3, 1)
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match="per device"):
        ShardedIndex.search_collapsed_combined(None, m[:2], 3, 1)
    with pytest.raises(NotImplementedError, match="per device"):
        ShardedIndex.search_batch_collapsed_combined(None, m[None, :2], 3, 1)


def test_collapsed_combined_op_maps_rows_to_embedding_ids():
    from svs_amd.matrix import collapsed_combined_op
    m = _unit(np.random.default_rng(2), 30, 8)
    idx = GroupCombineOracleIndex(m, 0, 100)
    idx.set_column(2, np.arange(30) // 4, 100)                   # rows 0 .. 3 carry 0, then groups of four
    arr = np.arange(30, dtype=np.int64) * 7 + 5                  # row r holds embedding id 7 r + 5
    for zero, groups in (("single", 4 + 7), ("group", 8)):
        native, finish = collapsed_combined_op(m[[9, 14]], 6, 2, "min", None, zero)
        used, (hits, g) = native(idx, None)
        assert used is idx and len(hits) == 6 and g == groups
        assert all(100 <= r < 130 for _, r, _ in hits)
        out, og = finish((used, (hits, g)), arr)
        assert og == groups and out == [(s, 7 * (r - 100) + 5, v) for s, r, v in hits]
        assert all(isinstance(x, int) for o in out for x in o[1:])
    # rows 9 and 14 are copies of the two vectors and lie in groups 2 and 3: under "max" those two groups lead, each
    # represented by the copy
    native, finish = collapsed_combined_op(m[[9, 14]], 2, 2)     # the defaults: "max", no weights, "single"
    out, _ = finish(native(idx, None), arr)
    assert sorted((e, v) for _, e, v in out) == [(7 * 9 + 5, 2), (7 * 14 + 5, 3)]
    idx.release()


def test_new_kernels_use_no_scratch_and_no_lds_and_the_combine_kernels_are_unchanged():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    with open(RES) as f:
        txt = f.read()
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)}
    names = _demangle([n for n in table if "multi_score_" in n or "cc_reduce" in n or "cc_mark" in n or "combine_" in n])
    # the multi-score pass: one instantiation per fused combine kernel; the group stage: two kernels
    for family, copies in (("multi_score_f32_kernel", 16), ("multi_score_f16_kernel", 8), ("multi_score_fp8_kernel", 6),
                           ("cc_reduce_kernel", 1), ("cc_mark_kernel", 1)):
        hits = [m for m, pretty in names.items() if f"svs::{family}" in pretty]
        assert len(hits) == copies, (family, sorted(names.values()))
        for h in hits:
            r = table[h]
            # (cc_reduce_kernel parks a few wave-uniform values in VGPR lanes -- an SGPR "spill" that touches no memory)
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{names[h]}: {r}"
            assert lds[h] == 0, (names[h], lds[h])
    # the kernels svs_index_search_combined runs keep their count and stay without scratch
    for family, copies in (("combine_f32_kernel", 16), ("combine_f16_kernel", 8), ("combine_fp8_kernel", 6), ("combine_scores_kernel", 1)):
        hits = [m for m, pretty in names.items() if f"svs::{family}" in pretty]
        assert len(hits) == copies, (family, sorted(names.values()))
        for h in hits:
            assert table[h]["scratch"] == 0 and table[h]["vgpr_spill"] == 0, f"{names[h]}: {table[h]}"

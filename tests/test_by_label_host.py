"""CPU: the per-level breakdown above the kernel -- level <-> label, emb id <-> row <-> doc mapping of
``KB.retrieve_by_level`` / ``AsyncKB.retrieve_by_level`` through a numpy double of DeviceIndex whose ``search_by_label``
is the numpy model of the definition (by_label_model.py); and the new kernels' resource report."""
import asyncio
import logging
import os
import re

import numpy as np
import pytest

import by_label_model
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources
from test_labels_host import LabelOracleIndex, _unit

import svs_amd
from svs_amd import multi as multi_mod


class ByLabelOracleIndex(LabelOracleIndex):
    """LabelOracleIndex whose ``search_by_label`` is the model over its own state."""

    calls = []          # (labels, min_score, n) of every search_by_label call, all instances

    def share(self):
        self._check()
        return ByLabelOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_by_label(self, q, labels, min_score=None, n=None):
        self._check()
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        labels = list(labels)
        ByLabelOracleIndex.calls.append((labels, min_score, n))
        l, s, r, t, _ = by_label_model.by_label(self.scores(q), self._st[2], self._st[1], labels, min_score, len(labels) if n is None else n)
        return list(zip(l.tolist(), s.astype(np.float64).tolist(), (r + self.row_offset).tolist(), t.tolist()))


def _kb(tmp_path, name, n_roots=10, d=16, seed=23):
    """A three-level KB: n_roots roots, 3 children each, 2 grandchildren per child.  {doc id: level}."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(400)] + [f"q {i}" for i in range(6)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=ByLabelOracleIndex)
    level, i = {}, 0
    with kb.bulk_add_docs() as add_doc:
        for _ in range(n_roots):
            root = add_doc(f"doc {i}"); level[root] = 0; i += 1
            for _ in range(3):
                child = add_doc(f"doc {i}", parent_id=root); level[child] = 1; i += 1
                for _ in range(2):
                    leaf = add_doc(f"doc {i}", parent_id=child); level[leaf] = 2; i += 1
    return kb, ef, table, level


def _expected(kb, table, query, min_score, levels):
    """The definition over the docs' own vectors: [(level, count, score, doc id)], best level first; a level's best
    doc is the one with the highest (score, embedding id)."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text, level FROM docs WHERE embedding IS NOT NULL").fetchall())
    m = np.array([table[t] for _, _, t, _ in rows], dtype=np.float32)
    s = np.dot(m, np.array(table[query], dtype=np.float32))
    out = []
    for lv in sorted(set(levels)):
        hit = [(s[i], i) for i, r in enumerate(rows) if r[3] == lv and (min_score is None or s[i] >= np.float32(min_score))]
        if hit:
            best = max(hit)
            out.append((best, lv, len(hit), float(best[0]), rows[best[1]][1]))
    return [o[1:] for o in sorted(out, reverse=True)]


def _got(res):
    return [(r["level"], r["count"], r["score"], r["doc"]["id"]) for r in res]


def test_retrieve_by_level_maps_levels_rows_and_docs(tmp_path, caplog):
    kb, ef, table, level = _kb(tmp_path, "a.sqlite")
    ByLabelOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_by_level("q 0")
    assert _got(got) == _expected(kb, table, "q 0", None, {0, 1, 2})
    assert sorted((r["level"], r["count"]) for r in got) == [(0, 10), (1, 30), (2, 60)]
    assert [r["score"] for r in got] == sorted((r["score"] for r in got), reverse=True)
    for r in got:
        assert r["doc"]["level"] == r["level"] == level[r["doc"]["id"]]
    assert set(got[0]) == {"level", "count", "score", "doc"} and set(got[0]["doc"]) == set(kb.retrieve("q 0", 1)[0]["doc"])
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving the best document of every level with query string: q 0", "got embedding for query!",
                     f"computed {len(level)} cosine similarities", "retrieved the best documents of 3 levels"]
    # levels=None read the store: the stored label of a level is level + 1; no cut-off, every label of the set asked for
    assert ByLabelOracleIndex.calls == [([1, 2, 3], None, None)]
    # the best doc of the best level is retrieve()'s first
    assert got[0]["doc"]["id"] == kb.retrieve("q 0", 1)[0]["doc"]["id"]
    # explicit levels go through the level -> label mapping; a level nobody has is absent
    for levels in (0, 2, (0, 2), [2, 2, 1], np.int64(1), range(3), range(7), [5]):
        ls = {int(levels)} if isinstance(levels, (int, np.integer)) else set(levels)
        assert _got(kb.retrieve_by_level("q 1", levels=levels)) == _expected(kb, table, "q 1", None, ls)
    assert ByLabelOracleIndex.calls[-1] == ([6], None, None) and ByLabelOracleIndex.calls[-2][0] == [1, 2, 3, 4, 5, 6, 7]
    assert kb.retrieve_by_level("q 1", levels=[5]) == [] and kb.retrieve_by_level("q 1", levels=[]) == []
    # counts under a cut-off: the docs of each level at or above it
    for cut in (0.0, 0.2, 0.45, 2.0, -1.0):
        got = kb.retrieve_by_level("q 2", cut)
        assert _got(got) == _expected(kb, table, "q 2", cut, {0, 1, 2})
        for r in got:
            assert r["count"] == sum(1 for x in kb.retrieve_at_level("q 2", 500, r["level"]) if x["score"] >= np.float32(cut))
    assert kb.retrieve_by_level("q 2", 2.0) == []
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        caplog.clear()
        kb.retrieve_by_level("q 2", 0.1, levels=(0, 2))
    assert [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"][0] == \
        "retrieving the best document of 2 levels with query string: q 2"
    kb.close()
    assert OracleIndex.live == 0


def test_levels_none_follows_the_store_and_the_column_is_shared_with_retrieve_at_level(tmp_path):
    kb, ef, table, level = _kb(tmp_path, "g.sqlite", n_roots=4)
    LabelOracleIndex.set_calls.clear()
    n = len(level)
    assert len(kb.retrieve_by_level("q 0")) == 3
    assert LabelOracleIndex.set_calls == [(0, n)]                # installed through ensure_labels, once
    kb.retrieve_at_level("q 0", 3, 1)
    kb.retrieve_by_level("q 1", 0.1)
    assert LabelOracleIndex.set_calls == [(0, n)]
    # a later bulk_add_docs adds a level: levels=None picks it up, and the new rows are labelled behind the append
    leaf = next(d for d, lv in level.items() if lv == 2)
    table["deep"] = table["q 3"]
    with kb.bulk_add_docs() as add_doc:
        deep = add_doc("deep", parent_id=leaf)
    level[deep] = 3
    got = kb.retrieve_by_level("q 3")
    assert _got(got) == _expected(kb, table, "q 3", None, {0, 1, 2, 3})
    assert (got[0]["level"], got[0]["count"], got[0]["doc"]["id"]) == (3, 1, deep)
    assert ByLabelOracleIndex.calls[-1][0] == [1, 2, 3, 4] and LabelOracleIndex.set_calls == [(0, n), (n, 1)]
    # deletions: the tombstoned doc leaves its level's count, and a level left empty leaves the result
    with kb.bulk_del_docs() as del_doc:
        del_doc(deep)
    del level[deep]
    got = kb.retrieve_by_level("q 3")
    assert _got(got) == _expected(kb, table, "q 3", None, {0, 1, 2}) and len(got) == 3
    kb.close()
    assert OracleIndex.live == 0


def test_arguments_are_checked(tmp_path):
    kb, ef, table, level = _kb(tmp_path, "v.sqlite", n_roots=2)
    with pytest.raises(ValueError, match="NaN"):
        kb.retrieve_by_level("q 0", float("nan"))
    for bad in (-1, [0, -2], 1.0, [True], "1", range(1025)):
        with pytest.raises(ValueError):
            kb.retrieve_by_level("q 0", levels=bad)
    assert len(kb.retrieve_by_level("q 0", levels=range(1024))) == 3      # 1,024 distinct levels are allowed

    async def run():
        akb = svs_amd.AsyncKB(kb.db.path, ef, index_factory=ByLabelOracleIndex)
        with pytest.raises(ValueError, match="NaN"):
            await akb.retrieve_by_level("q 0", float("nan"))
        for bad in (-1, range(1025)):
            with pytest.raises(ValueError):
                await akb.retrieve_by_level("q 0", levels=bad)
        await akb.close()

    asyncio.run(run())
    kb.close()


def test_async_retrieve_by_level_equals_sync(tmp_path, caplog):
    kb, ef, table, level = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    asks = [("q 0", None, None), ("q 1", 0.2, None), ("q 2", None, (0, 2)), ("q 3", 0.3, 1), ("q 4", 5.0, None), ("q 5", None, 9)]
    want = [_got(kb.retrieve_by_level(*a)) for a in asks]
    assert [len(w) for w in want][0] == 3 and want[4] == [] and want[5] == []
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=ByLabelOracleIndex)
        LabelOracleIndex.set_calls.clear()
        got = await asyncio.gather(*[akb.retrieve_by_level(*a) for a in asks])
        assert LabelOracleIndex.set_calls == [(0, len(level))]   # six concurrent tasks, one installation
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            await akb.retrieve_by_level("q 1", 0.2)
        async with akb.bulk_add_docs() as add_doc:
            table["late"] = table["q 5"]
            new = await add_doc("late")
        late = await akb.retrieve_by_level("q 5", levels=0)
        assert [(r["level"], r["count"], r["doc"]["id"]) for r in late] == [(0, 11, new)]
        await akb.close()
        return [_got(r) for r in got]

    assert asyncio.run(run()) == want
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving the best document of every level with query string: q 1", "got embedding for query!",
                     f"computed {len(level)} cosine similarities", f"retrieved the best documents of {len(want[1])} levels"]
    assert OracleIndex.live == 0


def test_multi_and_sharded_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[ByLabelOracleIndex(m[:20], 0, 0), ByLabelOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError):
        mi.search_by_label(m[0], [1])
    with pytest.raises(NotImplementedError):
        mi.search_batch_by_label(m[:2], [1])
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError):
        ShardedIndex.search_by_label(None, m[0], [1])
    with pytest.raises(NotImplementedError):
        ShardedIndex.search_batch_by_label(None, m[:2], [1])


def test_by_label_op_maps_rows_to_embedding_ids():
    from svs_amd.matrix import by_label_op
    m = _unit(np.random.default_rng(2), 30, 8)
    idx = ByLabelOracleIndex(m, 0, 100)
    idx.set_labels(np.arange(30) % 3 + 1, 100)
    arr = np.arange(30, dtype=np.int64) * 7 + 5                  # row r holds embedding id 7 r + 5
    native, finish = by_label_op(m[3], [1, 2, 3, 9], 0.0, 2)
    used, groups = native(idx, None)
    assert used is idx and len(groups) == 2
    out = finish((used, groups), arr)
    assert out == [(l, s, 7 * (r - 100) + 5, t) for l, s, r, t in groups]
    assert out[0][2] == 7 * 3 + 5 and all(isinstance(x, int) for o in out for x in (o[0], o[2], o[3]))
    idx.release()


def test_by_label_kernels_use_no_scratch_and_the_lds_their_tables_need():
    if not os.path.exists(RES):
        pytest.skip("no build reports (svs_amd/lib/build): run the build first")
    table = _resources(RES)
    names = _demangle([n for n in table if "by_label_" in n])
    with open(RES) as f:
        txt = f.read()
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", txt, re.S)}
    # reduce: the set (4 KiB) + a u64 best key and a u32 count per slot (12 KiB); final: best and total per slot, then
    # best, total and slot of every group (36 KiB) + the group counter
    for kernel, instances, lds_max in (("by_label_reduce_kernel", 2, 16 * 1024), ("by_label_final_kernel", 1, 36 * 1024 + 16)):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == instances, (kernel, sorted(names.values()))
        for h in hits:
            r = table[h]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{kernel}: {r}"
            assert 0 < lds[h] <= lds_max, (kernel, lds[h])
    assert len(names) == 3, sorted(names.values())

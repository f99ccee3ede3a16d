"""CPU: filtered retrieval above the kernel -- doc id -> emb id -> row mapping of ``KB.retrieve_within`` /
``AsyncKB.retrieve_within`` (through a numpy double of DeviceIndex), the shard split and merge of
``MultiDeviceIndex.search_batch_within``, and the gather kernels' resource report."""
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
from svs_amd.sharded import shard_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class WithinOracleIndex(OracleIndex):
    """OracleIndex that also answers ``search_within`` / ``search_batch_within``: the oracle on the sub-matrix of
    the live listed rows, positions mapped back to rows."""

    def __init__(self, matrix, device=0, row_offset=0, _shared=None, dtype="f32"):
        super().__init__(matrix, device, row_offset, _shared=_shared)
        self.dtype = dtype

    def share(self):
        self._check()
        return WithinOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_within(self, q, n, rows):
        self._check()
        assert isinstance(n, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        local = np.unique(np.asarray(rows, dtype=np.int64)) - self.row_offset
        if len(local) and (local[0] < 0 or local[-1] >= self.n):
            raise ValueError("row out of range")
        s = local[~self._st[1][local]]
        WithinOracleIndex.last_rows = s + self.row_offset
        return [(sc, int(s[p]) + self.row_offset) for sc, p in oracle.cpu_search(self._m[s], q, n)]

    def search_batch_within(self, queries, n, rows):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        res = [self.search_within(qq, n, rows) for qq in q]
        c = len(res[0]) if res else 0
        s = np.array([[a for a, _ in r] for r in res], dtype=np.float32).reshape(len(q), c)
        r = np.array([[b for _, b in r] for r in res], dtype=np.int64).reshape(len(q), c)
        return s, r


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _tree_kb(tmp_path, name, n_parents=4, per_parent=30, d=16, seed=3):
    """A KB of parents (no embedding: added with embed=False when supported, else embedded) and children."""
    rng = np.random.default_rng(seed)
    texts = [f"parent {p}" for p in range(n_parents)] + \
            [f"child {p}.{c}" for p in range(n_parents) for c in range(per_parent)] + [f"q {i}" for i in range(8)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=WithinOracleIndex)
    parents, children = [], {}
    with kb.bulk_add_docs() as add_doc:
        for p in range(n_parents):
            parents.append(add_doc(f"parent {p}"))
        for p in range(n_parents):
            children[parents[p]] = [add_doc(f"child {p}.{c}", parent_id=parents[p]) for c in range(per_parent)]
    return kb, ef, table, parents, children


def _expected(kb, table, query, n, doc_ids):
    """Oracle over the docs' own vectors: [(score, doc id)], order (score desc, emb id desc)."""
    with kb.db.transaction():
        rows = kb.db.conn.execute(
            f"SELECT id, embedding FROM docs WHERE id IN ({','.join('?' * len(doc_ids))})", list(doc_ids)).fetchall()
        text = dict(kb.db.conn.execute("SELECT id, text FROM docs").fetchall())
    rows = sorted((e, i) for i, e in rows if e is not None)   # by emb id: the order of the matrix rows
    m = np.array([table[text[i]] for _, i in rows], dtype=np.float32).reshape(len(rows), -1)
    q = np.array(table[query], dtype=np.float32)
    return [(s, rows[p][1]) for s, p in oracle.cpu_search(m, q, n)] if len(rows) else []


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_retrieve_within_maps_docs_to_rows_and_back(tmp_path, caplog):
    kb, ef, table, parents, children = _tree_kb(tmp_path, "w.sqlite")
    p = parents[1]
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_within("q 0", 10, children[p])
    assert _got(got) == _expected(kb, table, "q 0", 10, children[p])
    assert all(r["doc"]["parent_id"] == p for r in got) and len(got) == 10
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 10 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(children[p])} cosine similarities", "retrieved top 10 documents"]
    # same result shape as retrieve()
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])
    # the whole corpus listed == retrieve()
    every = [d for ch in children.values() for d in ch] + parents
    assert _got(kb.retrieve_within("q 1", 25, every)) == _got(kb.retrieve("q 1", 25))
    # one level of the tree; n past the subset; duplicates and any order
    assert _got(kb.retrieve_within("q 2", 3, parents)) == _expected(kb, table, "q 2", 3, parents)
    sub = children[parents[2]][:5]
    assert len(kb.retrieve_within("q 3", 50, sub[::-1] + sub)) == 5
    assert kb.retrieve_within("q 3", 0, sub) == [] and kb.retrieve_within("q 3", 5, []) == []
    kb.close()
    assert OracleIndex.live == 0


def test_retrieve_within_unknown_doc_and_docs_without_embedding(tmp_path):
    kb, ef, table, parents, children = _tree_kb(tmp_path, "u.sqlite")
    with pytest.raises(KeyError) as e:
        kb.retrieve_within("q 0", 5, [children[parents[0]][0], 987654])
    assert e.value.args == (987654,)
    # a doc whose embedding row is gone (stored without one) is skipped
    bare = children[parents[0]][0]
    with kb.db.transaction():
        emb = kb.db.conn.execute("SELECT embedding FROM docs WHERE id = ?", (bare,)).fetchone()[0]
        kb.db.conn.execute("UPDATE docs SET embedding = NULL WHERE id = ?", (bare,))
    listed = children[parents[0]][:6]
    got = kb.retrieve_within("q 1", 10, listed)
    assert bare not in [r["doc"]["id"] for r in got] and len(got) == 5
    assert _got(got) == _expected(kb, table, "q 1", 10, listed)
    assert emb is not None
    kb.close()


def test_retrieve_within_after_deletes_and_appends(tmp_path):
    kb, ef, table, parents, children = _tree_kb(tmp_path, "d.sqlite")
    kb.load()
    first = kb.embeddings_matrix.index
    p = parents[3]
    gone = children[p][::4]
    with kb.bulk_del_docs() as del_doc:
        for d in gone:
            del_doc(d)
    assert kb.embeddings_matrix.index is first            # tombstoned, not rebuilt
    live = [d for d in children[p] if d not in gone]
    got = kb.retrieve_within("q 4", 100, live)
    assert _got(got) == _expected(kb, table, "q 4", 100, live) and len(got) == len(live)
    with pytest.raises(KeyError):                          # a deleted doc is unknown now
        kb.retrieve_within("q 4", 5, gone[:1])
    table["late child"] = table["q 5"]                     # a new child equal to the query: it must come first
    with kb.bulk_add_docs() as add_doc:
        new = add_doc("late child", parent_id=p)
    assert kb.embeddings_matrix.index is first            # appended, not rebuilt
    got = kb.retrieve_within("q 5", 3, live + [new])
    assert got[0]["doc"]["id"] == new
    assert _got(got) == _expected(kb, table, "q 5", 3, live + [new])
    kb.close()


def test_async_retrieve_within_equals_sync(tmp_path):
    kb, ef, table, parents, children = _tree_kb(tmp_path, "a.sqlite")
    path = kb.db.path
    want = [_got(kb.retrieve_within(f"q {i}", 7, children[parents[i % 4]])) for i in range(6)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=WithinOracleIndex)
        got = await asyncio.gather(*[akb.retrieve_within(f"q {i}", 7, children[parents[i % 4]]) for i in range(6)])
        with pytest.raises(KeyError):
            await akb.retrieve_within("q 0", 3, [424242])
        await akb.close()
        return [_got(g) for g in got]

    assert asyncio.run(run()) == want
    assert OracleIndex.live == 0


def _fake_multi(m, g):
    bounds = [shard_bounds(m.shape[0], g, r) for r in range(g)]
    shards = [WithinOracleIndex(m[lo:hi], 0, lo) for lo, hi in bounds]
    return multi_mod.MultiDeviceIndex(None, _shards=shards, _bounds=bounds)


@pytest.mark.parametrize("rows_kind", ["spread", "one_shard", "underfilled", "masked_all", "empty"])
def test_multi_split_and_merge(rows_kind):
    rng = np.random.default_rng(7)
    m = _unit(rng, 400, 12)
    q = _unit(rng, 3, 12)
    mi = _fake_multi(m, 4)          # shards of 100 rows
    single = WithinOracleIndex(m)
    if rows_kind == "spread":
        rows = rng.choice(400, 150, replace=False)
    elif rows_kind == "one_shard":  # shards 0, 2 and 3 hold nothing
        rows = np.arange(120, 180)
    elif rows_kind == "underfilled":  # shard 3 holds 2 listed rows, below k
        rows = np.concatenate([np.arange(0, 60), np.arange(150, 200), [305, 399]])
    elif rows_kind == "masked_all":
        rows = np.arange(200, 210)
        mi.mask_rows(rows[:-3])
        single.mask_rows(rows[:-3])
    else:
        rows = np.array([], dtype=np.int64)
    for k in (1, 20, 1000):
        s, r = mi.search_batch_within(q, k, rows)
        es, er = single.search_batch_within(q, k, rows)
        assert r.shape == er.shape, (rows_kind, k)
        assert not np.isnan(s).any() and not (r < 0).any()
        # (rows exactly; the double scores each shard's sub-matrix with numpy, whose f32 sums move by an ulp with the
        #  matrix shape -- the GPU test checks the real shards bit for bit)
        assert np.array_equal(r, er) and np.allclose(s, es, rtol=0, atol=1e-6), (rows_kind, k)
    assert [r for _, r in mi.search_within(q[0], 5, rows)] == [r for _, r in single.search_within(q[0], 5, rows)]
    with pytest.raises(ValueError):
        mi.search_batch_within(q, 5, [400])
    mi.release()
    single.release()


def test_multi_within_skips_empty_shards():
    rng = np.random.default_rng(8)
    m = _unit(rng, 300, 8)
    mi = _fake_multi(m, 3)
    seen = []
    for s in mi._shards:
        orig = s.search_batch_within
        s.search_batch_within = (lambda o, sh: (lambda *a: (seen.append(sh), o(*a))[1]))(orig, s)
    mi.search_batch_within(_unit(rng, 1, 8), 4, [5, 6, 250])
    assert seen == [mi._shards[0], mi._shards[2]]
    mi.release()


def test_gather_kernels_use_no_scratch():
    if not os.path.exists(RES):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "gather_scores_kernel" in n])
    # 14 row geometries x 3 dtypes x (1 query, a group of queries)
    assert len(names) >= 84, sorted(names.values())
    for mangled, pretty in names.items():
        r = table[mangled]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{pretty}: {r}"

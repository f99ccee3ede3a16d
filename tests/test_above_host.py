"""CPU: threshold retrieval above the kernel -- emb id <-> row <-> doc mapping of ``KB.retrieve_above`` /
``AsyncKB.retrieve_above`` (through a numpy double of DeviceIndex whose ``search_above`` is the numpy model of the
definition), and the two new kernels' resource report."""
import asyncio
import logging
import os

import numpy as np
import pytest

import above_model
from fake_backend import OracleIndex
from oracle import svs_oracle as oracle
from test_kernel_resources import RES, _demangle, _resources

import svs_amd
from svs_amd import multi as multi_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AboveOracleIndex(OracleIndex):
    """OracleIndex that also answers ``search_above``: above_model on the oracle's score vector and the dead mask."""

    dtype = "f32"

    def share(self):
        self._check()
        return AboveOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_above(self, q, min_score, limit):
        self._check()
        assert isinstance(limit, int)
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        if min_score != min_score:
            raise ValueError("the cut-off of query 0 is NaN")
        rows, sc, total = above_model.above(oracle.cpu_scores(self._m, q), self._st[1], np.float32(min_score), limit)
        return list(zip(sc.astype(np.float64).tolist(), (rows + self.row_offset).tolist())), total


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_docs=120, d=16, seed=11):
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(n_docs)] + [f"q {i}" for i in range(6)]
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=AboveOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        docs = [add_doc(f"doc {i}") for i in range(n_docs)]
    return kb, ef, table, docs


def _expected(kb, table, query, cut, n):
    """The model over the docs' own vectors in embedding-id order (the order of the matrix rows): ([(score, doc id)], total)."""
    with kb.db.transaction():
        rows = kb.db.conn.execute("SELECT id, embedding, text FROM docs").fetchall()
    rows = sorted((e, i, t) for i, e, t in rows if e is not None)
    m = np.array([table[t] for _, _, t in rows], dtype=np.float32).reshape(len(rows), -1)
    s = oracle.cpu_scores(m, np.array(table[query], dtype=np.float32))
    r, sc, total = above_model.above(s, None, np.float32(cut), n)
    return [(float(a), rows[p][1]) for a, p in zip(sc, r)], total


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def _cut_with_total(kb, table, query, t):
    _, total = _expected(kb, table, query, -np.inf, 0)
    full, _ = _expected(kb, table, query, -np.inf, total)
    return full[t - 1][0]


def test_retrieve_above_maps_rows_to_docs(tmp_path, caplog):
    kb, ef, table, docs = _kb(tmp_path, "a.sqlite")
    cut = _cut_with_total(kb, table, "q 0", 9)
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got, total = kb.retrieve_above("q 0", cut, 20)
    exp, etotal = _expected(kb, table, "q 0", cut, 20)
    assert total == etotal == 9 and _got(got) == exp and len(got) == 9
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 20 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(docs)} cosine similarities", "retrieved top 20 documents"]
    # same result shape as retrieve(); everything above -inf, best first, is retrieve() of everything
    full = kb.retrieve("q 0", 1)
    assert set(got[0]) == set(full[0]) and set(got[0]["doc"]) == set(full[0]["doc"])
    every, total = kb.retrieve_above("q 1", -np.inf, len(docs))
    assert total == len(docs) and _got(every) == _got(kb.retrieve("q 1", len(docs)))
    # total > n: the list is cut by n, the total is not
    cut = _cut_with_total(kb, table, "q 2", 40)
    got, total = kb.retrieve_above("q 2", cut, 5)
    exp, _ = _expected(kb, table, "q 2", cut, 5)
    assert total == 40 and len(got) == 5 and _got(got) == exp
    # count only; nothing qualifies
    assert kb.retrieve_above("q 2", cut, 0) == ([], 40)
    assert kb.retrieve_above("q 2", 2.0, 10) == ([], 0)
    kb.close()
    assert OracleIndex.live == 0


def test_retrieve_above_nan_cutoff_and_docs_without_embedding(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "n.sqlite")
    with pytest.raises(ValueError):
        kb.retrieve_above("q 0", float("nan"), 5)
    # a doc stored without an embedding has no row: it is neither returned nor counted
    with kb.bulk_add_docs() as add_doc:
        bare = add_doc("q 3", no_embedding=True)        # (its text equals the query: it would come first)
    got, total = kb.retrieve_above("q 3", -np.inf, 500)
    exp, etotal = _expected(kb, table, "q 3", -np.inf, 500)
    assert total == etotal == len(docs) and _got(got) == exp
    assert bare not in [r["doc"]["id"] for r in got]
    kb.close()


def test_retrieve_above_after_deletes_and_appends(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "d.sqlite")
    kb.load()
    first = kb.embeddings_matrix.index
    best, _ = kb.retrieve_above("q 4", -np.inf, 6)
    gone = [r["doc"]["id"] for r in best[:3]]              # rows above every cut-off the others pass
    with kb.bulk_del_docs() as del_doc:
        for d in gone:
            del_doc(d)
    assert kb.embeddings_matrix.index is first              # tombstoned, not rebuilt
    got, total = kb.retrieve_above("q 4", -np.inf, 500)
    exp, etotal = _expected(kb, table, "q 4", -np.inf, 500)
    assert total == etotal == len(docs) - 3 and _got(got) == exp
    assert not set(gone) & {r["doc"]["id"] for r in got}
    assert [r["doc"]["id"] for r in got[:3]] == [r["doc"]["id"] for r in best[3:6]]
    table["late doc"] = table["q 4"]                        # equal to the query: score 1, first
    with kb.bulk_add_docs() as add_doc:
        new = add_doc("late doc")
    assert kb.embeddings_matrix.index is first              # appended, not rebuilt
    got, total = kb.retrieve_above("q 4", 0.99, 10)
    assert total == 1 and [r["doc"]["id"] for r in got] == [new]
    kb.close()


def test_async_retrieve_above_equals_sync(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    cuts = [_cut_with_total(kb, table, f"q {i}", 5 + 7 * i) for i in range(5)]
    want = [kb.retrieve_above(f"q {i}", cuts[i], 12) for i in range(5)]
    want = [(_got(r), t) for r, t in want]
    assert [t for _, t in want] == [5 + 7 * i for i in range(5)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=AboveOracleIndex)
        got = await asyncio.gather(*[akb.retrieve_above(f"q {i}", cuts[i], 12) for i in range(5)])
        with pytest.raises(ValueError):
            await akb.retrieve_above("q 0", float("nan"), 3)
        await akb.close()
        return [(_got(r), t) for r, t in got]

    assert asyncio.run(run()) == want
    assert OracleIndex.live == 0


def test_multi_search_above_is_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[AboveOracleIndex(m[:20], 0, 0), AboveOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError):
        mi.search_above(m[0], 0.5, 3)
    mi.release()


def test_above_kernels_use_no_scratch():
    if not os.path.exists(RES):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "above_" in n])
    for kernel in ("above_filter_kernel", "above_final_kernel"):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}(" in pretty]
        assert len(hits) == 1, (kernel, sorted(names.values()))
        r = table[hits[0]]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{kernel}: {r}"
    # neither is a score kernel by name: test_kernel_resources.py enumerates those
    assert not [p for p in names.values() if "gemv_" in p or "gemm_" in p or "gather_scores_kernel" in p]

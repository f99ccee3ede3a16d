"""CPU: diverse retrieval above the kernel -- emb id <-> row <-> doc mapping of ``KB.retrieve_diverse`` /
``AsyncKB.retrieve_diverse`` through a numpy double of DeviceIndex whose ``search_batch_diverse`` is the f64 model of the
definition (tests/diverse_model.py), the ``fetch_n`` default rule, the argument errors, and the two new kernels'
resource report."""
import asyncio
import logging
import os

import numpy as np
import pytest

import diverse_model as dm
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources

import svs_amd
from svs_amd import _native
from svs_amd.index import DIVERSE_MAX_FETCH, DeviceIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class DiverseOracleIndex(OracleIndex):
    """OracleIndex that also answers the diverse searches: the oracle's top fetch_k, then the model's greedy picks."""

    dtype = "f32"
    calls = []          # (n, fetch_k, lam) of every diverse search, any instance
    fail_next = False   # the next diverse search raises

    def share(self):
        self._check()
        return DiverseOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_batch_diverse(self, queries, n, fetch_k=None, lam=0.5):
        self._check()
        assert isinstance(n, int)
        if DiverseOracleIndex.fail_next:
            DiverseOracleIndex.fail_next = False
            raise RuntimeError("injected search failure")
        if not 0.0 <= float(lam) <= 1.0:
            raise ValueError(f"lam must lie in [0, 1], got {lam}")
        fk = DeviceIndex.diverse_fetch(n, fetch_k)
        DiverseOracleIndex.calls.append((n, fk, float(lam)))
        cs, cr = self.search_batch(queries, fk)
        count = min(max(n, 0), cs.shape[1])
        s = np.empty((cs.shape[0], count), dtype=np.float32)
        r = np.empty((cs.shape[0], count), dtype=np.int64)
        red = np.empty((cs.shape[0], count), dtype=np.float32)
        for i in range(cs.shape[0]):
            picks, reds = dm.greedy(cs[i], dm.gram64(self._m[cr[i] - self.row_offset]), count, lam)
            s[i], r[i], red[i] = cs[i][picks], cr[i][picks], reds
        return s, r, red

    def search_diverse(self, q, n, fetch_k=None, lam=0.5):
        q = np.asarray(q, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.d or self.n == 0:
            raise ValueError(f"shapes {self.shape} and {q.shape} not aligned")
        s, r, red = self.search_batch_diverse(q[None, :], n, fetch_k, lam)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist(), red[0].astype(np.float64).tolist()))


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_docs=120, d=16, seed=11):
    """Documents in near-copy families of three: what a diverse retrieval is for."""
    rng = np.random.default_rng(seed)
    base = _unit(rng, n_docs // 3, d)
    vecs = np.repeat(base, 3, axis=0) + 0.05 * rng.standard_normal((n_docs, d)).astype(np.float32)
    vecs = (vecs / np.linalg.norm(vecs, axis=1, keepdims=True)).astype(np.float32)
    table = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(n_docs)}
    for i, v in enumerate(_unit(rng, 6, d)):
        table[f"q {i}"] = [float(x) for x in v]

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=DiverseOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        docs = [add_doc(f"doc {i}") for i in range(n_docs)]
    return kb, ef, table, docs


def _expected(kb, table, query, n, fetch_k, lam):
    """The model over the docs' own vectors in embedding-id order (the order of the matrix rows):
    [(score, doc id, redundancy)] in pick order."""
    with kb.db.transaction():
        rows = kb.db.conn.execute("SELECT id, embedding, text FROM docs").fetchall()
    rows = sorted((e, i, t) for i, e, t in rows if e is not None)
    m = np.array([table[t] for _, _, t in rows], dtype=np.float32).reshape(len(rows), -1)
    oi = DiverseOracleIndex(m)
    try:
        got = oi.search_diverse(np.array(table[query], dtype=np.float32), n, fetch_k, lam)
    finally:
        oi.release()
        DiverseOracleIndex.calls.pop()
    return [(s, rows[r][1], red) for s, r, red in got]


def _got(res):
    return [(r["score"], r["doc"]["id"], r["redundancy"]) for r in res]


def test_binding_and_header_agree():
    assert "svs_index_search_diverse" in _native.SIGNATURES
    assert DIVERSE_MAX_FETCH == 1024
    with open(os.path.join(ROOT, "include", "svs_amd.h")) as f:
        assert "#define SVS_DIVERSE_MAX_FETCH 1024" in f.read()


def test_retrieve_diverse_maps_rows_to_docs_in_pick_order(tmp_path, caplog):
    kb, ef, table, docs = _kb(tmp_path, "a.sqlite")
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_diverse("q 0", 8, fetch_n=40, diversity=0.5)
    exp = _expected(kb, table, "q 0", 8, 40, 0.5)
    assert _got(got) == exp and len(got) == 8
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["retrieving 8 documents with query string: q 0", "got embedding for query!",
                     f"computed {len(docs)} cosine similarities", "retrieved top 8 documents"]
    # the shape of retrieve() plus 'redundancy'; pick order is not score order, and differs from plain retrieval
    plain = kb.retrieve("q 0", 8)
    assert set(got[0]) == set(plain[0]) | {"redundancy"} and set(got[0]["doc"]) == set(plain[0]["doc"])
    assert got[0]["redundancy"] == -np.inf and got[0]["doc"]["id"] == plain[0]["doc"]["id"]
    assert [r["doc"]["id"] for r in got] != [r["doc"]["id"] for r in plain]
    assert len({r["doc"]["id"] for r in got}) == 8
    # the near-copy families: plain retrieval returns whole families, the diverse one spreads over more of them
    fam = lambda res: {(r["doc"]["id"] - docs[0]) // 3 for r in res}   # noqa: E731
    assert len(fam(got)) > len(fam(plain))
    kb.close()
    assert OracleIndex.live == 0


def test_fetch_n_default_rule(tmp_path):
    assert [DeviceIndex.diverse_fetch(n) for n in (0, 1, 7, 8, 9, 100, 256, 300, 1024)] == [32, 32, 32, 32, 36, 400, 1024, 1024, 1024]
    assert DeviceIndex.diverse_fetch(5, 5) == 5 and DeviceIndex.diverse_fetch(5, 1024) == 1024
    kb, ef, table, docs = _kb(tmp_path, "f.sqlite")
    DiverseOracleIndex.calls.clear()
    kb.retrieve_diverse("q 1", 5)
    kb.retrieve_diverse("q 1", 20, diversity=0.25)
    kb.retrieve_diverse("q 1", 20, fetch_n=21, diversity=1.0)
    assert DiverseOracleIndex.calls == [(5, 32, 0.5), (20, 80, 0.75), (20, 21, 0.0)]
    # more results than documents: everything, once
    got = kb.retrieve_diverse("q 1", 500)
    assert sorted(r["doc"]["id"] for r in got) == sorted(docs)
    kb.close()


def test_diversity_zero_equals_retrieve(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "z.sqlite")
    for n in (1, 10, 32):
        got = kb.retrieve_diverse("q 2", n, diversity=0)
        plain = kb.retrieve("q 2", n)
        assert [(r["score"], r["doc"]) for r in got] == [(r["score"], r["doc"]) for r in plain]
    kb.close()


def test_argument_errors(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "e.sqlite")
    DiverseOracleIndex.calls.clear()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            kb.retrieve_diverse("q 0", 5, diversity=bad)
    with pytest.raises(ValueError):
        kb.retrieve_diverse("q 0", 1025)
    with pytest.raises(ValueError):
        kb.retrieve_diverse("q 0", 5, fetch_n=1025)
    with pytest.raises(ValueError):
        kb.retrieve_diverse("q 0", 5, fetch_n=4)
    assert DiverseOracleIndex.calls == []      # refused before any search
    kb.close()


def test_async_retrieve_diverse_equals_sync_and_releases_its_hold(tmp_path):
    kb, ef, table, docs = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    want = [_got(kb.retrieve_diverse(f"q {i}", 6 + i, diversity=0.2 * i)) for i in range(5)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=DiverseOracleIndex)
        got = await asyncio.gather(*[akb.retrieve_diverse(f"q {i}", 6 + i, diversity=0.2 * i) for i in range(5)])
        with pytest.raises(ValueError):
            await akb.retrieve_diverse("q 0", 2000)
        with pytest.raises(ValueError):
            await akb.retrieve_diverse("q 0", 5, diversity=2.0)
        live = OracleIndex.live
        DiverseOracleIndex.fail_next = True
        with pytest.raises(RuntimeError, match="injected"):
            await akb.retrieve_diverse("q 0", 5)
        assert OracleIndex.live == live        # the hold taken for the failed search is gone
        again = await akb.retrieve_diverse("q 0", 6, diversity=0.0)
        await akb.close()
        return [_got(r) for r in got], _got(again)

    got, again = asyncio.run(run())
    assert got == want and again == want[0]
    assert OracleIndex.live == 0


def test_diverse_kernels_use_no_scratch():
    if not os.path.exists(RES):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "diverse_" in n])
    for kernel, copies in (("diverse_gram_kernel", 3), ("diverse_pick_kernel", 1)):
        hits = [m for m, pretty in names.items() if f"svs::{kernel}" in pretty]
        assert len(hits) == copies, (kernel, sorted(names.values()))
        for h in hits:
            r = table[h]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{names[h]}: {r}"
    # neither is a score kernel by name: test_kernel_resources.py enumerates those
    assert not [p for p in names.values() if "gemv_" in p or "gemm_" in p or "gather_scores_kernel" in p]

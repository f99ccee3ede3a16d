"""CPU: combined retrieval above the kernel -- emb id <-> row <-> doc mapping of ``KB.retrieve_combined`` /
``AsyncKB.retrieve_combined`` through a numpy double of DeviceIndex whose ``search_batch_combined`` is the model of the
definition (tests/combine_model.py) over oracle scores; the three modes, the weights, the argument errors; the model
itself against hand-written cases; and the fused kernels' resource report."""
import asyncio
import logging
import os
import re

import numpy as np
import pytest

import combine_model as cm
from fake_backend import OracleIndex
from test_kernel_resources import RES, _demangle, _resources

import svs_amd
from svs_amd import _native
from svs_amd.index import COMBINE_MAX_VECTORS, COMBINE_OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class CombinedOracleIndex(OracleIndex):
    """OracleIndex that also answers combined searches: combine_model over the oracle's score vectors."""

    dtype = "f32"
    calls = []          # (m, n, op, weights or None) of every combined query, any instance
    fail_next = False   # the next combined search raises

    def share(self):
        self._check()
        return CombinedOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def search_batch_combined(self, vectors, n, op="max", weights=None):
        self._check()
        assert isinstance(n, int)
        if CombinedOracleIndex.fail_next:
            CombinedOracleIndex.fail_next = False
            raise RuntimeError("injected search failure")
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 3 or not 1 <= v.shape[1] <= COMBINE_MAX_VECTORS or v.shape[2] != self.d or op not in COMBINE_OPS:
            raise ValueError("bad combined query")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        if w is not None and (w.shape != v.shape[:2] or not np.isfinite(w).all()):
            raise ValueError("bad weights")
        dead = np.flatnonzero(self._st[1])
        k = min(max(n, 0), self.n - dead.size)
        s = np.empty((v.shape[0], k), dtype=np.float32)
        r = np.empty((v.shape[0], k), dtype=np.int64)
        for q in range(v.shape[0]):
            CombinedOracleIndex.calls.append((v.shape[1], n, op, None if w is None else w[q].tolist()))
            bits, rows, count = cm.top_k([self.scores(x) for x in v[q]], None if w is None else w[q], op, k, dead, self.row_offset)
            s[q], r[q] = bits.view(np.float32), rows
        return s, r, k

    def search_combined(self, vectors, n, op="max", weights=None):
        v = np.asarray(vectors, dtype=np.float32)
        if v.ndim != 2:
            raise ValueError(f"vectors must be (m, D), got shape {v.shape}")
        w = None if weights is None else np.asarray(weights, dtype=np.float32)[None, :]
        s, r, _ = self.search_batch_combined(v[None], n, op, w)
        return list(zip(s[0].astype(np.float64).tolist(), r[0].tolist()))


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _kb(tmp_path, name, n_docs=90, d=16, seed=13):
    rng = np.random.default_rng(seed)
    vecs = _unit(rng, n_docs, d)
    table = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(n_docs)}
    for i, v in enumerate(_unit(rng, 9, d)):
        table[f"q {i}"] = [float(x) for x in v]
    embed_calls = []

    async def ef(ts):
        embed_calls.append(list(ts))
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=CombinedOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        docs = [add_doc(f"doc {i}") for i in range(n_docs)]
    embed_calls.clear()
    return kb, ef, table, docs, embed_calls


def _expected(kb, table, queries, n, op, weights):
    """The model over the docs' own vectors in embedding-id order (the order of the matrix rows): [(score, doc id)]."""
    with kb.db.transaction():
        rows = kb.db.conn.execute("SELECT id, embedding, text FROM docs").fetchall()
    rows = sorted((e, i, t) for i, e, t in rows if e is not None)
    m = np.array([table[t] for _, _, t in rows], dtype=np.float32).reshape(len(rows), -1)
    s = [np.dot(m, np.array(table[q], dtype=np.float32)) for q in queries]
    bits, r, count = cm.top_k(s, None if weights is None else np.asarray(weights, dtype=np.float32), op, min(n, len(rows)))
    return [(float(x), rows[i][1]) for x, i in zip(bits.view(np.float32)[:count], r[:count])]


def _got(res):
    return [(r["score"], r["doc"]["id"]) for r in res]


def test_binding_and_header_agree():
    assert "svs_index_search_combined" in _native.SIGNATURES and "svs_internal_combined_scores" in _native.INTERNAL
    assert COMBINE_MAX_VECTORS == 8 and COMBINE_OPS == {"max": 0, "min": 1, "sum": 2}
    with open(os.path.join(ROOT, "include", "svs_amd.h")) as f:
        h = f.read()
    assert "#define SVS_COMBINE_MAX_VECTORS 8" in h
    assert re.search(r"SVS_COMBINE_MAX = 0, SVS_COMBINE_MIN = 1, SVS_COMBINE_SUM = 2", h)


def test_retrieve_combined_maps_rows_to_docs_in_every_mode(tmp_path, caplog):
    kb, ef, table, docs, embed_calls = _kb(tmp_path, "a.sqlite")
    qs = ["q 0", "q 1", "q 2"]
    CombinedOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.retrieve_combined(qs, 7)
    assert embed_calls == [qs]                                  # ONE embedding call
    assert CombinedOracleIndex.calls == [(3, 7, "max", None)]   # ONE combined query, mode "any" -> "max"
    assert _got(got) == _expected(kb, table, qs, 7, "max", None) and len(got) == 7
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == [f"retrieving 7 documents with 3 query strings: {qs}", "got embeddings for the queries!",
                     f"computed {len(docs)} x 3 cosine similarities", "retrieved top 7 documents"]
    plain = kb.retrieve("q 0", 7)
    assert set(got[0]) == set(plain[0]) and set(got[0]["doc"]) == set(plain[0]["doc"])
    w = [1.0, -0.5, 0.25]
    for mode, op in (("any", "max"), ("all", "min"), ("sum", "sum")):
        for weights in (None, w):
            CombinedOracleIndex.calls.clear()
            got = kb.retrieve_combined(qs, 12, mode=mode, weights=weights)
            assert CombinedOracleIndex.calls == [(3, 12, op, weights)]      # the weights pass through
            assert _got(got) == _expected(kb, table, qs, 12, op, weights), (mode, weights)
    # the three modes are three different rankings here, and "any" differs from a single query's
    ids = {m: [r["doc"]["id"] for r in kb.retrieve_combined(qs, 12, mode=m)] for m in ("any", "all", "sum")}
    assert ids["any"] != ids["all"] != ids["sum"] != ids["any"] and ids["any"] != [r["doc"]["id"] for r in kb.retrieve("q 0", 12)]
    # more results than documents: everything, once; eight queries are fine
    assert sorted(r["doc"]["id"] for r in kb.retrieve_combined(qs, 500, mode="sum")) == sorted(docs)
    assert len(kb.retrieve_combined([f"q {i}" for i in range(8)], 5)) == 5
    kb.close()
    assert OracleIndex.live == 0


def test_one_query_equals_retrieve(tmp_path):
    kb, ef, table, docs, _ = _kb(tmp_path, "o.sqlite")
    for n in (1, 10, 200):
        got, plain = kb.retrieve_combined(["q 3"], n), kb.retrieve("q 3", n)
        assert [(r["score"], r["doc"]) for r in got] == [(r["score"], r["doc"]) for r in plain]
    kb.close()


def test_removed_documents_never_come_back(tmp_path):
    kb, ef, table, docs, _ = _kb(tmp_path, "r.sqlite")
    qs = ["q 4", "q 5"]
    best = kb.retrieve_combined(qs, 3, mode="all")
    with kb.bulk_del_docs() as del_doc:
        del_doc(best[0]["doc"]["id"])
    got = kb.retrieve_combined(qs, 3, mode="all")
    assert best[0]["doc"]["id"] not in [r["doc"]["id"] for r in got]
    assert _got(got) == _expected(kb, table, qs, 3, "min", None)
    kb.close()


def test_argument_errors(tmp_path):
    kb, ef, table, docs, embed_calls = _kb(tmp_path, "e.sqlite")
    CombinedOracleIndex.calls.clear()
    for bad in ([], [f"q {i}" for i in range(9)]):
        with pytest.raises(ValueError):
            kb.retrieve_combined(bad, 5)
    with pytest.raises(ValueError):
        kb.retrieve_combined(["q 0"], 5, mode="mean")
    for w in ([1.0], [1.0, float("nan")], [1.0, float("inf")], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            kb.retrieve_combined(["q 0", "q 1"], 5, mode="sum", weights=w)
    assert CombinedOracleIndex.calls == [] and embed_calls == []      # refused before any embedding or search
    kb.close()


def test_async_retrieve_combined_equals_sync_and_releases_its_hold(tmp_path):
    kb, ef, table, docs, _ = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    cases = [(["q 0", "q 1"], 6, "any", None), (["q 2", "q 3", "q 4"], 9, "all", None), (["q 5", "q 6"], 4, "sum", [1.0, -1.0]),
             (["q 7"], 5, "any", None)]
    want = [_got(kb.retrieve_combined(q, n, mode=m, weights=w)) for q, n, m, w in cases]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=CombinedOracleIndex)
        got = await asyncio.gather(*[akb.retrieve_combined(q, n, mode=m, weights=w) for q, n, m, w in cases])
        with pytest.raises(ValueError):
            await akb.retrieve_combined([], 5)
        with pytest.raises(ValueError):
            await akb.retrieve_combined([f"q {i}" for i in range(9)], 5)
        with pytest.raises(ValueError):
            await akb.retrieve_combined(["q 0"], 5, mode="every")
        live = OracleIndex.live
        CombinedOracleIndex.fail_next = True
        with pytest.raises(RuntimeError, match="injected"):
            await akb.retrieve_combined(["q 0", "q 1"], 5)
        assert OracleIndex.live == live        # the hold taken for the failed search is gone
        one = await akb.retrieve_combined(["q 7"], 5)
        plain = await akb.retrieve("q 7", 5)
        await akb.close()
        return [_got(r) for r in got], _got(one), _got(plain)

    got, one, plain = asyncio.run(run())
    assert got == want and one == want[3] == plain
    assert OracleIndex.live == 0


# ---- the model itself -------------------------------------------------------------------------------------------------
def test_model_on_dyadic_values_is_exact():
    """Dyadic weights and scores: every product and sum is exact in f32, so the f64 arithmetic written out by hand is the
    f32 answer."""
    s = [np.array([0.5, -0.25, 1.0, 0.0], np.float32), np.array([0.25, 0.75, -1.0, 0.0], np.float32),
         np.array([-0.5, 0.125, 0.5, 0.0], np.float32)]
    w = np.array([2.0, -1.0, 0.5], np.float32)
    t = [[1.0, -0.5, 2.0, 0.0], [-0.25, -0.75, 1.0, -0.0], [-0.25, 0.0625, 0.25, 0.0]]        # w_j * s_j, by hand
    assert [x.tolist() for x in cm.terms(s, w)] == t
    assert cm.combine(s, w, "max").tolist() == [1.0, 0.0625, 2.0, 0.0]
    assert cm.combine(s, w, "min").tolist() == [-0.25, -0.75, 0.25, 0.0]
    assert cm.combine(s, w, "sum").tolist() == [0.5, -1.1875, 3.25, 0.0]
    assert cm.combine(s, None, "sum").tolist() == [0.25, 0.625, 0.5, 0.0]
    assert cm.combine(s[:1], None, "max").tolist() == s[0].tolist()
    # -0 folds onto +0 in max / min (the term of the zero score under the negative weight), bit for bit
    assert cm.combine(s[1:2], w[1:2], "max").view(np.uint32)[3] == 0 and cm.combine(s[1:2], w[1:2], "min").view(np.uint32)[3] == 0
    assert cm.combine(s[1:2], w[1:2], "sum").view(np.uint32)[3] == 0x80000000      # ... and stays -0 as a lone sum term
    # NaN is the largest key: first under max; under min only where every term is NaN
    n = [np.array([np.nan, np.nan, 1.0], np.float32), np.array([np.nan, 2.0, 3.0], np.float32)]
    assert np.isnan(cm.combine(n, None, "max")[:2]).all() and cm.combine(n, None, "max")[2] == 3.0
    mn = cm.combine(n, None, "min")
    assert np.isnan(mn[0]) and mn[1:].tolist() == [2.0, 1.0]
    assert np.isnan(cm.combine(n, None, "sum")[:2]).all()
    # top-k: (score desc, row desc), masked rows out, -inf / -1 past the count
    bits, rows, count = cm.top_k(s, w, "sum", 5, dead=[2], row_offset=10)
    assert count == 3 and rows.tolist() == [10, 13, 11, -1, -1]
    assert bits.view(np.float32).tolist() == [0.5, 0.0, -1.1875, -np.inf, -np.inf]


def test_model_sums_left_to_right():
    """((t0 + t1) + t2) is not (t0 + (t1 + t2)) in f32, and a fused multiply-add is not a multiplication and an addition:
    the model is the former of each pair."""
    one, eps = np.float32(1.0), np.float32(2.0 ** -24)
    s = [np.array([one]), np.array([eps]), np.array([eps])]
    assert cm.combine(s, None, "sum")[0] == one                          # (1 + e) + e: each e is rounded away
    assert np.float32(one + np.float32(eps + eps)) == np.float32(1.0 + 2.0 ** -23)    # 1 + (e + e) is not
    # w * s rounded, then added: with t0 = -(0.3f * 0.7f as f32) the two roundings give exactly 0; a fused multiply-add
    # would give the exact product's rounding error, -3.58e-09
    w, x = np.float32(0.3), np.float32(0.7)
    t0 = np.float32(-np.float32(w * x))
    got = cm.combine([np.array([t0]), np.array([x])], np.array([1.0, w], np.float32), "sum")[0]
    assert got == 0.0
    fused = np.float32(np.float64(w) * np.float64(x) + np.float64(t0))
    assert fused != 0.0 and abs(fused) < 1e-8


# ---- the build's resource report ----------------------------------------------------------------------------------------
def test_fused_kernels_use_no_scratch():
    """Every fused instantiation that ships: no scratch, no VGPR spill, at m = 8 as at m = 1 (the loop over the vectors
    is not unrolled: one vector's slice is in registers at a time); all three families are there."""
    if not os.path.exists(RES):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "combine_" in n])
    for family, copies in (("combine_f32_kernel", 16), ("combine_f16_kernel", 8), ("combine_fp8_kernel", 6), ("combine_scores_kernel", 1)):
        hits = [m for m, pretty in names.items() if f"svs::{family}" in pretty]
        assert len(hits) == copies, (family, sorted(names.values()))
        for h in hits:
            r = table[h]
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{names[h]}: {r}"
    # none is a single-query score kernel by name: test_kernel_resources.py enumerates those
    assert not [p for p in names.values() if "gemv_" in p or "gemm_" in p or "gather_scores_kernel" in p]

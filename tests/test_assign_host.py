"""CPU: nearest-vector assignment above the kernel -- emb id <-> row <-> doc mapping of ``KB.classify_documents`` /
``AsyncKB.classify_documents`` through a numpy double of DeviceIndex whose ``assign`` is the f64 model of the definition
(tests/assign_model.py), the argument errors, the multi-GPU wrappers, and the new kernel's resource report."""
import asyncio
import logging
import os
import subprocess

import numpy as np
import pytest

import assign_model as am
from fake_backend import OracleIndex
from test_kernel_resources import RES, ROOT, _demangle, _resources

import svs_amd
from svs_amd import _native
from svs_amd import multi as multi_mod
from svs_amd.index import ASSIGN_MAX_VECTORS, DeviceIndex


class AssignOracleIndex(OracleIndex):
    """OracleIndex that also answers ``assign``: the f64 model over its own rows and dead-row mask."""

    dtype = "f32"
    calls = []          # (c, labels is not None) of every assign call, any instance
    fail_next = False   # the next assign raises

    def share(self):
        self._check()
        return AssignOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def assign(self, vectors, labels=None, row0=None, nrows=None, scores=True):
        self._check()
        if AssignOracleIndex.fail_next:
            AssignOracleIndex.fail_next = False
            raise RuntimeError("injected assign failure")
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.d or self.n == 0 or v.shape[0] == 0:
            raise ValueError(f"shapes {self.shape} and {v.shape} not aligned")
        if v.shape[0] > ASSIGN_MAX_VECTORS:
            raise NotImplementedError(f"{v.shape[0]} vectors")
        AssignOracleIndex.calls.append((v.shape[0], labels is not None))
        r0 = 0 if row0 is None else row0 - self.row_offset
        r1 = self.n if nrows is None else r0 + nrows
        best, sc, counts = am.assign64(self._m[r0:r1], v, ~self._st[1][r0:r1])
        return best, (sc.astype(np.float32) if scores else None), counts


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


TOPICS = [f"topic {i}" for i in range(5)]


def _kb(tmp_path, name, d=16, seed=31):
    """A KB whose embedding ids are not contiguous in the matrix and which has deleted docs: 70 docs of which every
    ninth has no embedding, nine deletions (tombstones in the loaded matrix), then twenty more docs appended behind the
    gap, then three more deletions."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(90)] + TOPICS
    table = {t: [float(x) for x in v] for t, v in zip(texts, _unit(rng, len(texts), d))}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=AssignOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        docs = [add_doc(f"doc {i}", no_embedding=(i % 9 == 4)) for i in range(70)]
    kb.retrieve("topic 0", 1)                      # loads the matrix: what follows edits it in place
    with kb.bulk_del_docs() as del_doc:
        for i in (0, 3, 10, 11, 12, 30, 40, 55, 68):
            del_doc(docs[i])
    with kb.bulk_add_docs() as add_doc:
        docs += [add_doc(f"doc {i}") for i in range(70, 90)]
    with kb.bulk_del_docs() as del_doc:
        for i in (1, 75, 89):
            del_doc(docs[i])
    return kb, ef, table


def _expected(kb, table, topics):
    """The definition over the docs' own vectors in embedding-id order: (doc ids, topic, score f64, counts)."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text FROM docs WHERE embedding IS NOT NULL").fetchall())
    R = np.array([table[t] for _, _, t in rows], dtype=np.float32)
    V = np.array([table[t] for t in topics], dtype=np.float32)
    best, score, counts = am.assign64(R, V)
    return np.array([i for _, i, _ in rows], dtype=np.int64), best, score, counts


def _same(got, want):
    doc_ids, best, score, counts = want
    assert set(got) == {"doc_ids", "topic", "score", "counts"}
    assert got["doc_ids"].dtype == np.int64 and got["topic"].dtype == np.int32
    assert got["score"].dtype == np.float32 and got["counts"].dtype == np.int64
    assert np.array_equal(got["doc_ids"], doc_ids) and np.array_equal(got["topic"], best)
    assert np.array_equal(got["score"], score.astype(np.float32)) and np.array_equal(got["counts"], counts)
    assert got["counts"].sum() == len(doc_ids)


def test_binding_and_header_agree():
    assert "svs_index_assign" in _native.SIGNATURES and len(_native.SIGNATURES["svs_index_assign"][1]) == 10
    assert ASSIGN_MAX_VECTORS == 1024
    with open(os.path.join(ROOT, "include", "svs_amd.h")) as f:
        assert "#define SVS_ASSIGN_MAX_VECTORS 1024" in f.read()
    assert callable(DeviceIndex.assign)


def test_classify_documents_maps_rows_to_docs(tmp_path, caplog):
    kb, ef, table = _kb(tmp_path, "a.sqlite")
    AssignOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.classify_documents(TOPICS)
    want = _expected(kb, table, TOPICS)
    _same(got, want)
    # 90 docs, 8 + 0 without an embedding, 12 deleted -- one of them (doc 40) had none
    assert len(got["doc_ids"]) == 90 - 8 - 12 + 1 and len(set(got["topic"].tolist())) > 1
    n_rows = kb.embeddings_matrix.index.shape[0]
    assert n_rows > len(got["doc_ids"])          # the tombstoned rows are still in the matrix, and absent from the result
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["classifying every document by 5 topics", "got embeddings for the topics!",
                     f"computed {n_rows} x 5 cosine similarities", f"classified {len(got['doc_ids'])} documents"]
    assert AssignOracleIndex.calls == [(5, False)]      # one native call, and the label column is not touched
    # topic order is the caller's: a permutation of the topics permutes the answer
    perm = [3, 0, 4, 1, 2]
    got2 = kb.classify_documents([TOPICS[p] for p in perm])
    assert np.array_equal(np.array(perm)[got2["topic"]], got["topic"]) and np.array_equal(got2["counts"], got["counts"][perm])
    # a fresh KB over the same store (the matrix rebuilt from storage, nothing tombstoned) answers the same
    path = kb.db.path
    kb.close()
    kb2 = svs_amd.KB(path, ef, index_factory=AssignOracleIndex)
    _same(kb2.classify_documents(TOPICS), want)
    assert kb2.embeddings_matrix.index.shape[0] == len(want[0])
    kb2.close()
    assert OracleIndex.live == 0


def test_argument_errors(tmp_path):
    kb, ef, table = _kb(tmp_path, "e.sqlite")
    AssignOracleIndex.calls.clear()
    with pytest.raises(ValueError):
        kb.classify_documents([])
    with pytest.raises(ValueError, match="1025"):
        kb.classify_documents(["topic 0"] * 1025)
    assert AssignOracleIndex.calls == []      # refused before anything is embedded or assigned

    async def run():
        akb = svs_amd.AsyncKB(kb.db.path, ef, index_factory=AssignOracleIndex)
        with pytest.raises(ValueError):
            await akb.classify_documents([])
        with pytest.raises(ValueError):
            await akb.classify_documents(["topic 1"] * 1025)
        await akb.close()

    asyncio.run(run())
    assert AssignOracleIndex.calls == []
    assert kb.classify_documents(["topic 2"] * 1024)["counts"][0] > 0     # 1,024 topics are allowed; copies tie to the first
    kb.close()


def test_async_classify_documents_equals_sync_and_releases_its_hold(tmp_path, caplog):
    kb, ef, table = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    want = _expected(kb, table, TOPICS)
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=AssignOracleIndex)
        AssignOracleIndex.calls.clear()
        with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
            got = await akb.classify_documents(TOPICS)
        assert AssignOracleIndex.calls == [(5, False)]
        both = await asyncio.gather(akb.classify_documents(TOPICS[:2]), akb.classify_documents(TOPICS))
        live = OracleIndex.live
        AssignOracleIndex.fail_next = True
        with pytest.raises(RuntimeError, match="injected"):
            await akb.classify_documents(TOPICS)
        assert OracleIndex.live == live        # the hold taken for the failed call is gone
        # a deletion behind the loaded matrix: the doc leaves the answer and its topic's count
        gone = int(got["doc_ids"][5])
        async with akb.bulk_del_docs() as del_doc:
            await del_doc(gone)
        after = await akb.classify_documents(TOPICS)
        await akb.close()
        return got, both, gone, after

    got, both, gone, after = asyncio.run(run())
    _same(got, want)
    _same(both[1], want)
    assert len(both[0]["counts"]) == 2 and both[0]["counts"].sum() == len(want[0])
    keep = got["doc_ids"] != gone
    assert np.array_equal(after["doc_ids"], got["doc_ids"][keep]) and np.array_equal(after["topic"], got["topic"][keep])
    assert after["counts"].sum() == keep.sum() and after["counts"][got["topic"][5]] == got["counts"][got["topic"][5]] - 1
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == ["classifying every document by 5 topics", "got embeddings for the topics!",
                     f"computed {len(want[0])} x 5 cosine similarities", f"classified {len(want[0])} documents"]
    assert OracleIndex.live == 0


def test_assign_op_maps_rows_to_embedding_ids_and_drops_tombstones():
    from svs_amd.matrix import _Lookup, assign_op
    rng = np.random.default_rng(2)
    m, v = _unit(rng, 30, 8), _unit(rng, 4, 8)
    idx = AssignOracleIndex(m, 0, 100)
    lookup = _Lookup(np.arange(30, dtype=np.int64) * 7 + 5)      # row r holds embedding id 7 r + 5
    native, finish = assign_op(v)
    ids, best, scores, counts = finish(native(idx, lookup), lookup.arr)
    wb, ws, wc = am.assign64(m, v)
    assert np.array_equal(ids, lookup.arr) and np.array_equal(best, wb) and np.array_equal(counts, wc)
    assert ids.dtype == np.int64 and best.dtype == np.int32 and scores.dtype == np.float32 and counts.dtype == np.int64
    dead = np.array([0, 13, 29])
    idx.mask_rows(dead + 100)
    lookup.dead = dead
    ids, best, scores, counts = finish(native(idx, lookup), lookup.arr)
    live = np.ones(30, dtype=bool)
    live[dead] = False
    assert np.array_equal(ids, lookup.arr[live]) and np.array_equal(best, wb[live])
    assert np.array_equal(counts, np.bincount(wb[live], minlength=4)) and counts.sum() == 27
    # a removal the device has seen and the lookup read before it has not: the counts follow the rows returned
    lookup.dead = dead[:2]
    ids, best, scores, counts = finish(native(idx, lookup), lookup.arr)
    assert len(ids) == 28 and counts.sum() == 28 and np.array_equal(counts, np.bincount(best, minlength=4))
    idx.release()


def test_multi_and_sharded_calls_are_not_implemented():
    m = _unit(np.random.default_rng(1), 40, 8)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[AssignOracleIndex(m[:20], 0, 0), AssignOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError):
        mi.assign(m[:3])
    with pytest.raises(NotImplementedError):
        mi.assign(m[:3], labels=[1, 2, 3])
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError):
        ShardedIndex.assign(None, m[:3])


def test_assign_kernel_uses_no_scratch():
    if not os.path.exists(RES):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "assign_" in n])
    hits = [m for m, pretty in names.items() if "svs::assign_rows_kernel" in pretty]
    assert len(hits) == len(names) and hits, sorted(names.values())
    for h in hits:
        r = table[h]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{names[h]}: {r}"
    # the three dtypes, each with its sweep widths
    for dt in (0, 1, 2):
        assert [p for p in names.values() if f"assign_rows_kernel<{dt}, " in p], (dt, sorted(names.values()))
    # not a score kernel by name: test_kernel_resources.py enumerates those
    assert not [p for p in names.values() if "gemv_" in p or "gemm_" in p or "gather_" in p]

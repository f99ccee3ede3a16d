"""CPU: per-label sums and k-means above the kernels -- ``KB.cluster_documents`` / ``AsyncKB.cluster_documents`` through a
numpy double of DeviceIndex whose ``assign`` and ``label_sums`` are the models of their definitions
(tests/assign_model.py, tests/label_sums_model.py) and whose ``kmeans`` is DeviceIndex's own loop; the argument errors,
the multi-GPU wrappers, header / signature / hook consistency, and the new kernels' resource report."""
import asyncio
import logging
import os
import re
import subprocess

import numpy as np
import pytest

import assign_model as am
import label_sums_model as lm
from fake_backend import OracleIndex
from test_kernel_resources import RES, ROOT, _demangle, _resources

import svs_amd
from svs_amd import _native
from svs_amd import multi as multi_mod
from svs_amd.index import ASSIGN_MAX_VECTORS, LABELS_MAX_SET, DeviceIndex, _centroids, labels_u32

D = 16
K = 4


class ClusterOracleIndex(OracleIndex):
    """OracleIndex that also answers ``assign``, ``label_sums`` and ``stored_rows`` from the models, over its own rows and
    dead-row mask; ``kmeans`` is the product's loop run over them."""

    dtype = "f32"
    calls = []          # ("assign", c, labels is not None) / ("label_sums", L, row_labels is not None) of every call
    fail_next = False   # the next label_sums raises
    grow_next = None    # rows the next assign appends to the index right after it has answered (a concurrent append)

    def share(self):
        self._check()
        return ClusterOracleIndex(None, self.device, self.row_offset, _shared=self._st)

    def _range(self, row0, nrows):
        r0 = 0 if row0 is None else row0 - self.row_offset
        return r0, (self.n if nrows is None else r0 + nrows)

    def stored_rows(self, row0=0, nrows=None):
        self._check()
        return np.array(self._m[row0:(self.n if nrows is None else row0 + nrows)], dtype=np.float32)

    def assign(self, vectors, labels=None, row0=None, nrows=None, scores=True):
        self._check()
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.d or self.n == 0 or v.shape[0] == 0:
            raise ValueError(f"shapes {self.shape} and {v.shape} not aligned")
        ClusterOracleIndex.calls.append(("assign", v.shape[0], labels is not None))
        r0, r1 = self._range(row0, nrows)
        best, sc, counts = am.assign64(self._m[r0:r1], v, ~self._st[1][r0:r1])
        if ClusterOracleIndex.grow_next is not None:
            rows, ClusterOracleIndex.grow_next = ClusterOracleIndex.grow_next, None
            self.append(rows)
        return best, (sc.astype(np.float32) if scores else None), counts

    def _extent(self):
        return self.row_offset, self.n, self.d

    _stored_rows_at = DeviceIndex._stored_rows_at

    def label_sums(self, labels, row_labels=None, row0=None, nrows=None, sums=True):
        self._check()
        if ClusterOracleIndex.fail_next:
            ClusterOracleIndex.fail_next = False
            raise RuntimeError("injected label_sums failure")
        lab = labels_u32(labels)
        ClusterOracleIndex.calls.append(("label_sums", len(lab), row_labels is not None))
        r0, r1 = self._range(row0, nrows)
        rl = np.zeros(r1 - r0, dtype=np.uint32) if row_labels is None else labels_u32(row_labels)
        if len(rl) != r1 - r0:
            raise ValueError(f"{len(rl)} row labels for {r1 - r0} rows")
        s, c = lm.replay(self._m[r0:r1], rl, ~self._st[1][r0:r1], lab)
        return (s if sums else None), c

    kmeans = DeviceIndex.kmeans


def _planted(rng, n, d=D, k=K, noise=0.05):
    """n unit rows around k orthogonal directions (row i around direction i % k) and the directions."""
    dirs = np.eye(d, dtype=np.float64)[:k]
    x = dirs[np.arange(n) % k] + noise * rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), dirs


def _kb(tmp_path, name, seed=31):
    """The KB shape of test_assign_host.py: embedding ids that are not contiguous in the matrix and deleted docs -- 70
    docs of which every ninth has no embedding, nine deletions (tombstones in the loaded matrix), then twenty more docs
    appended behind the gap, then three more deletions.  Doc i sits near planted direction i % K."""
    rng = np.random.default_rng(seed)
    texts = [f"doc {i}" for i in range(90)] + ["q"]
    vecs, _ = _planted(rng, len(texts))
    table = {t: [float(x) for x in v] for t, v in zip(texts, vecs)}

    async def ef(ts):
        return [table[t] for t in ts]

    kb = svs_amd.KB(str(tmp_path / name), ef, index_factory=ClusterOracleIndex)
    with kb.bulk_add_docs() as add_doc:
        docs = [add_doc(f"doc {i}", no_embedding=(i % 9 == 4)) for i in range(70)]
    kb.retrieve("q", 1)                            # loads the matrix: what follows edits it in place
    with kb.bulk_del_docs() as del_doc:
        for i in (0, 3, 10, 11, 12, 30, 40, 55, 68):
            del_doc(docs[i])
    with kb.bulk_add_docs() as add_doc:
        docs += [add_doc(f"doc {i}") for i in range(70, 90)]
    with kb.bulk_del_docs() as del_doc:
        for i in (1, 75, 89):
            del_doc(docs[i])
    return kb, ef, table


def _docs(kb, table):
    """(doc ids, planted cluster, vectors) of the docs that have an embedding, in embedding-id order."""
    with kb.db.transaction():
        rows = sorted(kb.db.conn.execute("SELECT embedding, id, text FROM docs WHERE embedding IS NOT NULL").fetchall())
    ids = np.array([i for _, i, _ in rows], dtype=np.int64)
    planted = np.array([int(t.split()[1]) % K for _, _, t in rows])
    return ids, planted, np.array([table[t] for _, _, t in rows], dtype=np.float32)


def _check_clustering(got, ids, planted, vecs):
    assert set(got) == {"doc_ids", "cluster", "score", "counts", "centroids", "iterations"}
    assert got["doc_ids"].dtype == np.int64 and got["cluster"].dtype == np.int32 and got["score"].dtype == np.float32
    assert got["counts"].dtype == np.int64 and got["centroids"].dtype == np.float32 and isinstance(got["iterations"], int)
    assert np.array_equal(got["doc_ids"], ids)                    # the doc <-> row mapping; tombstoned docs are absent
    assert got["counts"].sum() == len(ids) and got["centroids"].shape == (K, D)
    assert np.array_equal(got["counts"], np.bincount(got["cluster"], minlength=K))
    # the planted clusters, up to relabelling
    pairs = set(zip(planted.tolist(), got["cluster"].tolist()))
    assert len(pairs) == K and len({p for p, _ in pairs}) == K and len({c for _, c in pairs}) == K, sorted(pairs)
    # a centroid is the normalised mean of its docs' vectors
    for c in range(K):
        mean = vecs[got["cluster"] == c].astype(np.float64).mean(axis=0)
        assert np.allclose(got["centroids"][c], mean / np.linalg.norm(mean), rtol=0, atol=1e-6)
    assert 1 <= got["iterations"] <= 10


def test_binding_header_and_hook_agree():
    sig = _native.SIGNATURES["svs_index_label_sums"]
    assert len(sig[1]) == 8
    assert "svs_internal_label_sums_kernel_ms" in _native.INTERNAL
    with open(os.path.join(ROOT, "include", "svs_amd.h")) as f:
        header = f.read()
    assert "#define SVS_LABEL_SUMS_CHUNK 256" in header and lm.CHUNK == 256
    decl = re.search(r"int32_t svs_index_label_sums\((.*?)\);", header, flags=re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 8
    with open(os.path.join(ROOT, "svs_amd", "csrc", "internal.h")) as f:
        assert "int32_t svs_internal_label_sums_kernel_ms(double* out);" in f.read()
    lib = _native.load()
    assert hasattr(lib, "svs_index_label_sums") and hasattr(lib, "svs_internal_label_sums_kernel_ms")
    for name in ("label_sums", "label_means", "kmeans"):
        assert callable(getattr(DeviceIndex, name))
    assert callable(svs_amd.KB.cluster_documents) and callable(svs_amd.AsyncKB.cluster_documents)


def test_cluster_documents_maps_rows_to_docs(tmp_path, caplog):
    kb, ef, table = _kb(tmp_path, "a.sqlite")
    ids, planted, vecs = _docs(kb, table)
    ClusterOracleIndex.calls.clear()
    with caplog.at_level(logging.INFO, logger="svs_amd.kb"):
        got = kb.cluster_documents(K, seed=3)
    _check_clustering(got, ids, planted, vecs)
    assert len(got["doc_ids"]) == 90 - 8 - 12 + 1
    n_rows = kb.embeddings_matrix.index.shape[0]
    assert n_rows > len(got["doc_ids"])          # the tombstoned rows are still in the matrix, and absent from the result
    lines = [r.getMessage() for r in caplog.records if r.name == "svs_amd.kb"]
    assert lines == [f"clustering every document into {K} clusters", f"ran {got['iterations']} k-means iterations over {n_rows} embeddings",
                     f"clustered {len(got['doc_ids'])} documents"]
    # assign then label_sums per iteration, the sums labelled by the assignment; the label column is never written
    calls = ClusterOracleIndex.calls
    assert calls[0] == ("assign", K, False) and ("label_sums", K, True) in calls
    assert all(c in (("assign", K, False), ("label_sums", K, True)) for c in calls)
    assert sum(c[0] == "label_sums" for c in calls) == got["iterations"]
    # one seed, one answer
    again = kb.cluster_documents(K, seed=3)
    for key in ("doc_ids", "cluster", "score", "counts", "centroids"):
        assert np.array_equal(again[key], got[key]), key
    # a fresh KB over the same store (the matrix rebuilt from storage, nothing tombstoned) finds the same partition
    path = kb.db.path
    kb.close()
    kb2 = svs_amd.KB(path, ef, index_factory=ClusterOracleIndex)
    _check_clustering(kb2.cluster_documents(K, seed=3), ids, planted, vecs)
    assert kb2.embeddings_matrix.index.shape[0] == len(ids)
    kb2.close()
    assert OracleIndex.live == 0


def test_async_cluster_documents_equals_sync_and_releases_its_hold(tmp_path):
    kb, ef, table = _kb(tmp_path, "s.sqlite")
    path = kb.db.path
    ids, planted, vecs = _docs(kb, table)
    kb.close()
    kb = svs_amd.KB(path, ef, index_factory=ClusterOracleIndex)
    want = kb.cluster_documents(K, seed=3)
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef, index_factory=ClusterOracleIndex)
        got = await akb.cluster_documents(K, seed=3)
        live = OracleIndex.live
        ClusterOracleIndex.fail_next = True
        with pytest.raises(RuntimeError, match="injected"):
            await akb.cluster_documents(K)
        assert OracleIndex.live == live        # the hold taken for the failed call is gone
        gone = int(got["doc_ids"][5])
        async with akb.bulk_del_docs() as del_doc:
            await del_doc(gone)
        after = await akb.cluster_documents(K, seed=3)
        await akb.close()
        return got, gone, after

    got, gone, after = asyncio.run(run())
    _check_clustering(got, ids, planted, vecs)
    for key in ("doc_ids", "cluster", "score", "counts", "centroids"):
        assert np.array_equal(got[key], want[key]), key
    keep = ids != gone
    _check_clustering(after, ids[keep], planted[keep], vecs[keep])
    assert OracleIndex.live == 0


def test_cluster_op_drops_tombstones_and_keeps_counts_consistent():
    from svs_amd.matrix import _Lookup, cluster_op
    rng = np.random.default_rng(2)
    m, _ = _planted(rng, 40)
    idx = ClusterOracleIndex(m, 0, 100)
    lookup = _Lookup(np.arange(40, dtype=np.int64) * 7 + 5)      # row r holds embedding id 7 r + 5
    native, finish = cluster_op(K, 10, 1)
    ids, best, scores, counts, cent, ran = finish(native(idx, lookup), lookup.arr)
    assert np.array_equal(ids, lookup.arr) and counts.sum() == 40 and cent.shape == (K, D) and ran >= 1
    assert ids.dtype == np.int64 and best.dtype == np.int32 and scores.dtype == np.float32 and counts.dtype == np.int64
    dead = np.array([0, 13, 39])
    idx.mask_rows(dead + 100)
    lookup.dead = dead
    ids, best, scores, counts, cent, ran = finish(native(idx, lookup), lookup.arr)
    live = np.ones(40, dtype=bool)
    live[dead] = False
    assert np.array_equal(ids, lookup.arr[live]) and counts.sum() == 37 and np.array_equal(counts, np.bincount(best, minlength=K))
    # the tombstoned rows have no weight in the centroids
    for c in range(K):
        mean = m[live][best == c].astype(np.float64).mean(axis=0)
        assert np.allclose(cent[c], mean / np.linalg.norm(mean), rtol=0, atol=1e-6)
    lookup.dead = dead[:2]      # a removal the device has seen and the lookup read before it has not
    ids, best, scores, counts, cent, ran = finish(native(idx, lookup), lookup.arr)
    assert len(ids) == 38 and counts.sum() == 38 and np.array_equal(counts, np.bincount(best, minlength=K))
    idx.release()


def test_rows_appended_during_the_loop_take_no_part():
    """An append that lands between the assign and the label_sums of one iteration (another thread of an AsyncKB, another
    owner of the handle): the loop keeps the row range it began with, in every call."""
    from svs_amd.matrix import _Lookup, cluster_op
    rng = np.random.default_rng(8)
    m, _ = _planted(rng, 60)
    extra, _ = _planted(rng, 7)
    first = m[:K].copy()          # rows 0 .. K - 1 sit near directions 0 .. K - 1
    quiet = ClusterOracleIndex(m, 0, 100)
    want = quiet.kmeans(K, init=first)
    quiet.release()
    idx = ClusterOracleIndex(m, 0, 100)
    ClusterOracleIndex.calls.clear()
    ClusterOracleIndex.grow_next = extra
    got = idx.kmeans(K, init=first, write_labels=True)
    assert ClusterOracleIndex.grow_next is None and idx.n == 67
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g, w)
    assert len(got[1]) == 60 and got[3].sum() == 60 and got[4] == want[4]
    assert ClusterOracleIndex.calls[-1] == ("assign", K, True)          # the labelling call covers the same 60 rows
    # through the mapped op: the lookup has grown with the index, the answer maps the rows the loop covered
    lookup = _Lookup(np.arange(67, dtype=np.int64) * 3 + 1)
    ClusterOracleIndex.grow_next = extra
    native, finish = cluster_op(K, 10, 1)
    ids, best, scores, counts, cent, ran = finish(native(idx, lookup), lookup.arr)
    assert idx.n == 74 and np.array_equal(ids, lookup.arr[:67]) and len(best) == 67 and counts.sum() == 67
    idx.release()


def test_kmeans_takes_any_integer_and_refuses_the_rest():
    m, _ = _planted(np.random.default_rng(4), 30)
    idx = ClusterOracleIndex(m, 0, 0)
    a = idx.kmeans(np.int64(3), iterations=np.int32(2), init=m[:3])
    b = idx.kmeans(3, iterations=2, init=m[:3])
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    for bad in (2.0, "3", None):
        with pytest.raises(ValueError, match="integers"):
            idx.kmeans(bad)
        with pytest.raises(ValueError, match="integers"):
            idx.kmeans(3, iterations=bad)
    # the first centroids are the stored values of the drawn rows, whatever the order and spacing of the draw
    rows = np.array([29, 0, 1, 17, 2, 28])
    assert np.array_equal(idx._stored_rows_at(rows), m[rows]) and np.array_equal(idx._stored_rows_at(rows, gap=0), m[rows])
    idx.release()


def test_kmeans_update_rule():
    sums = np.array([[2.0, 0.0], [0.0, 0.0], [3.0, 4.0], [0.0, 0.0]])
    counts = np.array([2, 0, 5, 3], dtype=np.int64)
    prev = np.array([[9, 9], [8, 8], [7, 7], [6, 6]], dtype=np.float32)
    sph = _centroids(sums, counts, prev, True)
    assert sph.dtype == np.float32 and sph.tolist() == [[1.0, 0.0], [8.0, 8.0], [np.float32(0.6), np.float32(0.8)], [6.0, 6.0]]
    flat = _centroids(sums, counts, prev, False)
    assert flat.tolist() == [[1.0, 0.0], [8.0, 8.0], [np.float32(0.6), np.float32(0.8)], [6.0, 6.0]]


def test_argument_errors(tmp_path):
    m, _ = _planted(np.random.default_rng(4), 30)
    idx = ClusterOracleIndex(m, 0, 0)
    ClusterOracleIndex.calls.clear()
    for bad in (0, -1, ASSIGN_MAX_VECTORS + 1):
        with pytest.raises(ValueError):
            idx.kmeans(bad)
    with pytest.raises(ValueError):
        idx.kmeans(3, iterations=0)
    with pytest.raises(ValueError):
        idx.kmeans(31)                                  # more clusters than rows to draw from
    with pytest.raises(ValueError):
        idx.kmeans(3, init=np.zeros((3, D + 1), dtype=np.float32))
    with pytest.raises(ValueError):
        idx.kmeans(3, init=np.zeros((2, D), dtype=np.float32))
    assert ClusterOracleIndex.calls == []              # refused before anything runs
    idx.release()
    # DeviceIndex.label_sums refuses bad labels before it touches the library
    for bad in ([-1], [2 ** 32], [0.5]):
        with pytest.raises(ValueError):
            DeviceIndex.label_sums(None, bad)
        with pytest.raises(ValueError):
            DeviceIndex.label_sums(None, [1], row_labels=bad)
    kb, ef, table = _kb(tmp_path, "e.sqlite")
    ClusterOracleIndex.calls.clear()
    for bad in (0, 1025):
        with pytest.raises(ValueError, match=str(bad)):
            kb.cluster_documents(bad)
    with pytest.raises(ValueError):
        kb.cluster_documents(3, iterations=0)
    assert ClusterOracleIndex.calls == []

    async def run():
        akb = svs_amd.AsyncKB(kb.db.path, ef, index_factory=ClusterOracleIndex)
        with pytest.raises(ValueError):
            await akb.cluster_documents(0)
        with pytest.raises(ValueError):
            await akb.cluster_documents(1025)
        await akb.close()

    asyncio.run(run())
    assert ClusterOracleIndex.calls == []
    kb.close()
    assert LABELS_MAX_SET == ASSIGN_MAX_VECTORS == 1024


def test_multi_and_sharded_calls_are_not_implemented():
    m, _ = _planted(np.random.default_rng(1), 40)
    mi = multi_mod.MultiDeviceIndex(None, _shards=[ClusterOracleIndex(m[:20], 0, 0), ClusterOracleIndex(m[20:], 0, 20)],
                                    _bounds=[(0, 20), (20, 40)])
    with pytest.raises(NotImplementedError, match="per device"):
        mi.label_sums([0, 1])
    with pytest.raises(NotImplementedError, match="per device"):
        mi.label_means([0, 1], row_labels=np.zeros(40, dtype=np.uint32))
    with pytest.raises(NotImplementedError, match="per device"):
        mi.kmeans(3)
    mi.release()
    from svs_amd.sharded import ShardedIndex
    with pytest.raises(NotImplementedError, match="per device"):
        ShardedIndex.label_sums(None, [0])
    with pytest.raises(NotImplementedError, match="per device"):
        ShardedIndex.label_means(None, [0])
    with pytest.raises(NotImplementedError, match="per device"):
        ShardedIndex.kmeans(None, 3)


def test_label_sums_kernels_use_no_scratch_and_the_sum_kernel_fits_two_waves():
    if not os.path.exists(RES):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    table = _resources(RES)
    names = _demangle([n for n in table if "label_sums_" in n])
    pretty = sorted(names.values())
    for kernel in ("hist", "scan", "plan", "scatter", "fold"):
        assert [p for p in pretty if f"svs::label_sums_{kernel}_kernel(" in p], (kernel, pretty)
    for dt in (0, 1, 2):
        assert [p for p in pretty if f"svs::label_sums_chunk_kernel<{dt}>" in p], (dt, pretty)
    assert len(names) == 8, pretty
    for mangled, p in names.items():
        r = table[mangled]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, f"{p}: {r}"
        if "chunk_kernel" in p:
            assert r["vgpr"] + r["agpr"] <= 256, f"{p}: {r} -- two waves per SIMD need <= 256 registers"
    # not a score kernel by name: test_kernel_resources.py enumerates those
    assert not [p for p in pretty if "gemv_" in p or "gemm_" in p or "gather_" in p]

"""GPU: filtered retrieval (svs_index_search_rows, gather.h) -- top-k over a caller-given subset of the rows.

Every answer is compared with the reference's get_top_k(np.dot(M[S], q), k) (src/svs/util.py:190-203) on the STORED
rows and query, S = the live listed rows ascending, positions mapped back to S, through assert_topk_parity with f64
truth; every call also asserts, through svs_internal_last_launches, that the gather kernel ran over exactly |S| rows
and that nothing scored the whole corpus."""
import asyncio
import threading

import numpy as np
import pytest

from compare import assert_topk_parity
from oracle import svs_oracle as oracle

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-6, "f16": 2e-6, "fp8": 5e-6}   # tests/test_batch_kernels_gpu.py: TOL, TOL_FP8_GEMV
SORT_CAP = 4096


def _unit_rows(rng, n, d):
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


def _gather_launches(n_corpus, n_listed):
    from svs_amd import _native
    launches = _native.last_launches()
    gathers = [rec for rec in launches if rec[0].startswith("gather_scores_kernel")]
    assert gathers, launches
    assert all(rec[1] == n_listed for rec in gathers), launches
    if n_listed != n_corpus:
        assert all(rec[1] != n_corpus for rec in launches), launches
    return gathers


def _check(idx, stored, q_stored, q, k, rows, label, tol, dead=None):
    """One search_within call against the oracle on the stored sub-matrix."""
    lo = idx.row_offset
    s_all = np.unique(np.asarray(rows, dtype=np.int64))
    if dead is not None:
        s_all = s_all[~dead[s_all - lo]]
    S = s_all
    got = idx.search_within(q, k, rows)
    want_count = min(max(k, 0), len(S))
    assert len(got) == want_count, (label, len(got), want_count)
    if len(S) and k > 0:
        _gather_launches(idx.n, len(S))
    if not len(S) or k <= 0:
        return got
    sub = stored[S - lo]
    exp = oracle.cpu_search(sub, q_stored, k)
    truth = sub.astype(np.float64) @ q_stored.astype(np.float64)
    got_rows = np.array([r for _, r in got], dtype=np.int64)
    pos = np.searchsorted(S, got_rows)
    assert np.all(pos < len(S)) and np.array_equal(S[np.minimum(pos, len(S) - 1)], got_rows), f"{label}: row outside S"
    assert_topk_parity([s for s, _ in got], pos, [s for s, _ in exp], [p for _, p in exp], truth64=truth,
                       label=label, score_atol=tol)
    assert np.max(np.abs(np.array([s for s, _ in got]) - truth[pos])) <= tol, label
    return got


_CORPORA = {}


def _corpus(d):
    if d not in _CORPORA:
        n = 60_000 if d >= 3072 else 100_000
        rng = np.random.default_rng(d)
        _CORPORA.clear()
        _CORPORA[d] = (_unit_rows(rng, n, d), _unit_rows(rng, 4, d))
    return _CORPORA[d]


def _subsets(n, rng):
    return {
        "1pct": rng.choice(n, n // 100, replace=False),
        "50pct": np.sort(rng.choice(n, n // 2, replace=False)),
        "all": np.arange(n),
        "block": np.arange(n // 3, n // 3 + 7_000),
        "single": np.array([n // 2 + 7]),
        "ends": np.array([0, n - 1]),
        "unsorted_dups": np.concatenate([rng.choice(n, 3000), rng.choice(n, 3000)]),
    }


@pytest.mark.parametrize("d", [1536, 3072, 768, 100])
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_parity_across_shapes_and_subsets(gpu, dtype, d):
    from svs_amd import DeviceIndex
    m, qs = _corpus(d)
    n = m.shape[0]
    idx = DeviceIndex(m, dtype=dtype)
    stored = m if dtype == "f32" else idx.stored_rows()
    rng = np.random.default_rng(d + 1)
    q = qs[0]
    q_stored = idx.stored_query(q)
    for name, rows in _subsets(n, rng).items():
        for k in (1, 100, 5000, 10 ** 6):
            _check(idx, stored, q_stored, q, k, rows, f"{dtype} d={d} {name} k={k}", TOL[dtype])
    idx.release()


def test_one_million_rows_f32(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(99)
    m = _unit_rows(rng, 1_000_000, 1536)
    q = _unit_rows(rng, 1, 1536)[0]
    idx = DeviceIndex(m)
    for name, rows in (("1pct", rng.choice(1_000_000, 10_000, replace=False)),
                       ("high rows", np.arange(990_000, 1_000_000)),
                       ("block", np.arange(400_000, 520_000))):
        _check(idx, m, q, q, 100, rows, f"1M {name}", TOL["f32"])
    idx.release()


def test_tombstones(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(5)
    m = _unit_rows(rng, 20_000, 768)
    q = _unit_rows(rng, 1, 768)[0]
    idx = DeviceIndex(m)
    rows = rng.choice(20_000, 3_000, replace=False)
    masked = rows[::3]
    idx.mask_rows(masked)
    dead = np.zeros(20_000, dtype=bool)
    dead[masked] = True
    for k in (10, 2_000, 5_000):
        got = _check(idx, m, q, q, k, rows, f"masked k={k}", TOL["f32"], dead=dead)
        assert not set(r for _, r in got) & set(masked.tolist())
        assert len(got) == min(k, 3_000 - len(masked))
    assert idx.search_within(q, 10, masked) == []
    s, r = idx.search_batch_within(np.stack([q, q]), 10, masked)
    assert s.shape == (2, 0) and r.shape == (2, 0)
    idx.release()


def test_row_offset_is_global(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(6)
    m = _unit_rows(rng, 10_000, 1536)
    q = _unit_rows(rng, 1, 1536)[0]
    off = 1_000_000
    idx = DeviceIndex(m, row_offset=off)
    rows = off + rng.choice(10_000, 500, replace=False)
    got = _check(idx, m, q, q, 50, rows, "row_offset", TOL["f32"])
    assert all(r >= off for _, r in got)
    with pytest.raises(ValueError):
        idx.search_within(q, 5, [3])            # a local row is out of range
    with pytest.raises(ValueError):
        idx.search_within(q, 5, [off + 10_000])
    idx.release()


@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_batches_are_bit_identical_to_single_queries(gpu, dtype):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(7)
    m = _unit_rows(rng, 30_000, 1536)
    Q = _unit_rows(rng, 40, 1536)
    idx = DeviceIndex(m, dtype=dtype)
    rows = rng.choice(30_000, 6_000, replace=False)
    solo = [idx.search_batch_within(Q[i:i + 1], 100, rows) for i in range(40)]
    for nq in (3, 16, 40):
        s, r = idx.search_batch_within(Q[:nq], 100, rows)
        g = _gather_launches(30_000, 6_000)
        assert sum(rec[2] for rec in g) == nq
        for i in range(nq):
            assert np.array_equal(s[i], solo[i][0][0]) and np.array_equal(r[i], solo[i][1][0]), (dtype, nq, i)
    idx.release()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_full_list_equals_search(gpu, dtype):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(8)
    m = _unit_rows(rng, 50_000, 1536)
    Q = _unit_rows(rng, 5, 1536)
    idx = DeviceIndex(m, dtype=dtype)
    stored = m if dtype == "f32" else idx.stored_rows()
    every = np.arange(50_000)
    s1, r1 = idx.search_batch_within(Q, 200, every)
    s2, r2 = idx.search_batch(Q, 200)
    for i in range(5):
        truth = stored.astype(np.float64) @ idx.stored_query(Q[i]).astype(np.float64)
        assert_topk_parity(s1[i], r1[i], s2[i], r2[i], truth64=truth, label=f"{dtype} full q{i}", score_atol=2e-6)
    got = idx.search_within(Q[0], 200, every)
    want = idx.search(Q[0], 200)
    assert_topk_parity([a for a, _ in got], [b for _, b in got], [a for a, _ in want], [b for _, b in want],
                       truth64=stored.astype(np.float64) @ idx.stored_query(Q[0]).astype(np.float64), score_atol=2e-6)
    idx.release()


def test_errors(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(9)
    m = _unit_rows(rng, 1_000, 64)
    q = _unit_rows(rng, 1, 64)[0]
    idx = DeviceIndex(m)
    with pytest.raises(ValueError):
        idx.search_within(q, 5, [1_000])
    with pytest.raises(ValueError):
        idx.search_within(q, 5, [-1])
    with pytest.raises(ValueError):
        idx.search_within(np.zeros(63, dtype=np.float32), 5, [1, 2])
    assert idx.search_within(q, 5, []) == []
    assert idx.search_within(q, 0, [1, 2]) == []
    idx.release()


def test_concurrent_calls_on_one_handle(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(10)
    m = _unit_rows(rng, 40_000, 1536)
    Q = _unit_rows(rng, 8, 1536)
    idx = DeviceIndex(m)
    lists = [rng.choice(40_000, s, replace=False) for s in (100, 2_000, 20_000, 40_000)]
    jobs = [("within", i % 8, i % 4) for i in range(24)] + [("search", i % 8, None) for i in range(8)]
    solo = {}
    for kind, qi, li in jobs:
        solo[(kind, qi, li)] = idx.search_within(Q[qi], 50, lists[li]) if kind == "within" else idx.search(Q[qi], 50)
    errors = []

    def worker(t):
        try:
            for r in range(3):
                for j, (kind, qi, li) in enumerate(jobs):
                    if (j + t + r) % 4:
                        continue
                    got = idx.search_within(Q[qi], 50, lists[li]) if kind == "within" else idx.search(Q[qi], 50)
                    if got != solo[(kind, qi, li)]:
                        errors.append((kind, qi, li))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:5]
    idx.release()


def test_multi_device_split_is_bit_identical(gpu):
    from svs_amd import DeviceIndex, MultiDeviceIndex
    rng = np.random.default_rng(11)
    m = _unit_rows(rng, 30_000, 768)
    Q = _unit_rows(rng, 3, 768)
    one = DeviceIndex(m)
    two = MultiDeviceIndex(m, devices=[0, 0])
    lists = {"spread": rng.choice(30_000, 4_000, replace=False),
             "second shard only": np.arange(20_000, 21_000),
             "underfilled": np.concatenate([np.arange(0, 3_000), [29_998, 29_999]])}
    for name, rows in lists.items():
        for k in (1, 100, 5_000):
            a = one.search_batch_within(Q, k, rows)
            b = two.search_batch_within(Q, k, rows)
            assert a[0].shape == b[0].shape, (name, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, k)
            assert not np.isnan(b[0]).any() and (b[1] >= 0).all()
    assert one.search_within(Q[0], 10, lists["spread"]) == two.search_within(Q[0], 10, lists["spread"])
    one.release()
    two.release()


def _tree(tmp_path, name, n_parents=5, per_parent=40, d=256, seed=12):
    rng = np.random.default_rng(seed)
    texts = [f"parent {p}" for p in range(n_parents)] + \
            [f"child {p}.{c}" for p in range(n_parents) for c in range(per_parent)] + [f"q {i}" for i in range(4)]
    vecs = _unit_rows(rng, len(texts), d)
    table = {t: [float(x) for x in v] for t, v in zip(texts, vecs)}

    async def ef(ts):
        return [table[t] for t in ts]

    return texts, table, ef


def _oracle_docs(table, text_of, doc_ids, query, n):
    ids = sorted(doc_ids)
    mat = np.array([table[text_of[i]] for i in ids], dtype=np.float32)
    q = np.array(table[query], dtype=np.float32)
    return [(s, ids[p]) for s, p in oracle.cpu_search(mat, q, n)], mat.astype(np.float64) @ q.astype(np.float64), ids


def _check_kb(got, table, text_of, doc_ids, query, n, parent):
    exp, truth, ids = _oracle_docs(table, text_of, doc_ids, query, n)
    assert all(r["doc"]["parent_id"] == parent for r in got)
    pos_got = [ids.index(r["doc"]["id"]) for r in got]
    assert_topk_parity([r["score"] for r in got], pos_got, [s for s, _ in exp], [ids.index(i) for _, i in exp],
                       truth64=truth, score_atol=2e-6)


def test_kb_and_async_kb_retrieve_within(gpu, tmp_path):
    import svs_amd
    texts, table, ef = _tree(tmp_path, "kb")
    path = str(tmp_path / "kb.sqlite")
    kb = svs_amd.KB(path, ef)
    parents, children = [], {}
    with kb.bulk_add_docs() as add_doc:
        for p in range(5):
            parents.append(add_doc(f"parent {p}"))
        for p in range(5):
            children[parents[p]] = [add_doc(f"child {p}.{c}", parent_id=parents[p]) for c in range(40)]
    text_of = {}
    with kb.db.transaction():
        for i, t in kb.db.conn.execute("SELECT id, text FROM docs"):
            text_of[i] = t
    P = parents[2]
    got = kb.retrieve_within("q 0", 10, children[P])
    assert len(got) == 10
    _check_kb(got, table, text_of, children[P], "q 0", 10, P)
    _gather_launches(kb.embeddings_matrix.index.n, 40)
    # a deleted child stops appearing; an added one appears without a rebuild
    first = kb.embeddings_matrix.index
    gone = [r["doc"]["id"] for r in got[:3]]
    with kb.bulk_del_docs() as del_doc:
        for d_ in gone:
            del_doc(d_)
    live = [c for c in children[P] if c not in gone]
    got = kb.retrieve_within("q 0", 10, live)
    assert not set(gone) & {r["doc"]["id"] for r in got}
    _check_kb(got, table, text_of, live, "q 0", 10, P)
    table["late"] = table["q 1"]
    with kb.bulk_add_docs() as add_doc:
        late = add_doc("late", parent_id=P)
    text_of[late] = "late"
    assert kb.embeddings_matrix.index is first
    got = kb.retrieve_within("q 1", 5, live + [late])
    assert got[0]["doc"]["id"] == late
    _check_kb(got, table, text_of, live + [late], "q 1", 5, P)
    with pytest.raises(KeyError):
        kb.retrieve_within("q 1", 5, [10 ** 9])
    listing = [[c for c in children[parents[i]] if c not in gone] for i in range(4)]
    want = [[(r["score"], r["doc"]["id"]) for r in kb.retrieve_within(f"q {i}", 7, listing[i])] for i in range(4)]
    kb.close()

    async def run():
        akb = svs_amd.AsyncKB(path, ef)
        res = await asyncio.gather(*[akb.retrieve_within(f"q {i}", 7, listing[i]) for i in range(4)])
        await akb.close()
        return [[(r["score"], r["doc"]["id"]) for r in g] for g in res]

    assert asyncio.run(run()) == want

"""GPU: threshold search (svs_index_search_above; svs_amd/csrc/above.h) against its definition.

The truth for membership and bits is ``idx.scores(q)`` (svs_index_scores_n: the same kernel) fed to the numpy model
(above_model.py): rows, order, score bits, counts and totals must be EQUAL.  Shapes: 40,003 rows (no multiple of 4,
five filter workgroups of 8,192 scores, more than CAND_CAP = 32,768) of 64 unit-norm Gaussian elements.  Cut-offs are
taken from the score vector so that the total is exactly what a case needs: the cut-off is the t-th best live score."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import above_model
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, D = 40003, 64
DTYPES = ["f32", "f16", "fp8"]
TOL = {"f32": 2e-6, "f16": 2e-6, "fp8": 5e-6}     # test_single_kernels_gpu.py's, per dtype
SORT_CAP, CAND_CAP = 4096, 32768


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261)
    return _unit(rng, N, D), _unit(rng, 5, D)


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    m, q = data
    idx = svs_amd.DeviceIndex(m, dtype=request.param)
    s = [idx.scores(qq) for qq in q]          # the reference, computed once, never written
    for v in s:
        v.setflags(write=False)
    yield SimpleNamespace(idx=idx, s=s, m=m, q=q, dtype=request.param)
    idx.release()


def _pick(c, t, dead=None, scores=None):
    """(query number, cut-off) with exactly t qualifying live rows: the first query whose t-th and (t+1)-th best live
    scores differ (a tie there -- one in a thousand -- would make the total t impossible)."""
    for qi in range(len(c.q)):
        try:
            return qi, above_model.cut_for_total((scores or c.s)[qi], dead, t)
        except AssertionError:
            continue
    raise AssertionError(f"every query ties at rank {t}")


def _check(got, exp, what):
    s, r, total = got
    er, es, etotal = exp
    assert total == etotal, (what, total, etotal)
    assert r.tolist() == er.tolist(), what
    # (score bits; a NaN comes back as THE quiet NaN, whatever its sign and payload were: key_score, as in every search)
    canon = lambda a: np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).tolist()
    assert canon(s) == canon(es), what


def _names():
    return [k for k, _, _ in _native.last_launches()]


def _assert_path(nq, reruns, rows=N):
    """This thread's last call: one filter per query over `rows` scores, one score pass per query plus one per re-run, and
    the exact top-k stage only in the re-runs."""
    rec = _native.last_launches()
    names = [k for k, _, _ in rec]
    assert [(k, r, q) for k, r, q in rec if k == "above_filter_kernel"] == [("above_filter_kernel", rows, 1)] * nq
    assert names.count("gemv") == nq + reruns, names
    kernels = [k for k in names if k not in ("gemv", "above_filter_kernel") and not k.startswith(("select_", "keys_", "bitonic"))]
    assert len(kernels) == nq + reruns, names                         # (the score kernel behind every "gemv" entry)
    stage = [k for k in names if k.startswith(("select_", "keys_", "bitonic"))]
    assert len(stage) == reruns, names


def _raw(idx, q, cuts, limit, out_s, out_r, counts, totals, d=None, nq=None):
    q = np.ascontiguousarray(q, dtype=np.float32)
    cuts = np.ascontiguousarray(cuts, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    return idx._lib.svs_index_search_above(idx._handle(), q.ctypes.data, q.shape[0] if nq is None else nq, q.shape[1] if d is None else d,
                                           cuts.ctypes.data, limit, p(out_s), p(out_r), p(counts), p(totals))


@pytest.mark.parametrize("t", [0, 1, 255, 256, 257, 4096, 4097, 32768, 32769, N])
def test_totals(case, t):
    c = case
    qi, cut = (0, np.float32(-np.inf)) if t == N else _pick(c, t)
    got = c.idx.search_batch_above(c.q[qi:qi + 1], [cut], N)[0]
    _assert_path(1, 0 if t <= SORT_CAP else 1)       # (limit = n: the wanted prefix is the whole list)
    exp = above_model.above(c.s[qi], None, cut, N)
    assert exp[2] == t
    _check(got, exp, (c.dtype, t))


@pytest.mark.parametrize("limit,t,reruns,stage", [(10, 5000, 0, None), (10, 33000, 1, "select_window_hist_kernel"),
                                                  (5000, 6000, 1, "keys_build_kernel")])
def test_limits(case, limit, t, reruns, stage):
    c = case
    qi, cut = _pick(c, t)
    got = c.idx.search_batch_above(c.q[qi:qi + 1], [cut], limit)[0]
    _assert_path(1, reruns)
    assert ([k for k in _names() if k.startswith(("select_", "keys_"))] or [None]) == [stage]
    exp = above_model.above(c.s[qi], None, cut, limit)
    assert exp[2] == t and len(exp[0]) == limit
    _check(got, exp, (c.dtype, limit, t))


def test_count_only_and_limit_past_n(case):
    c = case
    qi, cut = _pick(c, 300)
    # limit = 0 (and a negative one): totals, counts 0, null result pointers at the C level
    for limit in (0, -5):
        counts, totals = np.full(1, 77, dtype=np.int32), np.full(1, -1, dtype=np.int64)
        assert _raw(c.idx, c.q[qi:qi + 1], [cut], limit, None, None, counts, totals) == 0, _native.last_error()
        assert counts.tolist() == [0] and totals.tolist() == [300]
        _assert_path(1, 0)
    # ... also when the list overflows: still exact, still no re-run
    qj, big = _pick(c, 33000)
    counts, totals = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    assert _raw(c.idx, c.q[qj:qj + 1], [big], 0, None, None, counts, totals) == 0
    assert counts.tolist() == [0] and totals.tolist() == [33000]
    _assert_path(1, 0)
    assert c.idx.search_above(c.q[qi], float(cut), 0) == ([], 300)
    # totals may be NULL; limit > n: the caller's stride is the limit, entries past the count are not touched
    limit = N + 1000
    out_s, out_r = np.full((1, limit), -7.0, dtype=np.float32), np.full((1, limit), -7, dtype=np.int64)
    counts = np.zeros(1, dtype=np.int32)
    assert _raw(c.idx, c.q[qi:qi + 1], [cut], limit, out_s, out_r, counts, None) == 0
    er, es, _ = above_model.above(c.s[qi], None, cut, limit)
    assert counts.tolist() == [300] and out_r[0, :300].tolist() == er.tolist()
    assert out_s[0, :300].view(np.uint32).tolist() == es.view(np.uint32).tolist()
    assert (out_s[0, 300:] == -7.0).all() and (out_r[0, 300:] == -7).all()
    _check(c.idx.search_batch_above(c.q[qi:qi + 1], [cut], limit)[0], (er, es, 300), c.dtype)


def test_tombstones_and_compaction(data, gpu, case):
    m, q = data
    dtype = case.dtype
    s = case.s[0]
    rng = np.random.default_rng(3)
    dead = rng.random(N) < 0.05
    best = int(np.argmax(s))
    dead[[0, N - 1, best]] = True           # the ends, and a row above every cut-off used here
    dead[64:96] = True                      # a whole bitmap word
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        idx.mask_rows(np.nonzero(dead)[0])
        n_live = int((~dead).sum())
        # -inf: exactly the live rows (their masked score would pass; the bitmap keeps them out), through the re-run
        got = idx.search_batch_above(q[:1], [-np.inf], N)[0]
        _assert_path(1, 1)
        _check(got, above_model.above(s, dead, -np.inf, N), dtype)
        assert got[2] == n_live and not dead[got[1]].any()
        # device-complete zone: totals exclude dead rows; the best row is dead and stays out
        for t, limit in ((700, N), (5000, 20), (n_live, 0)):
            cut = np.float32(-np.inf) if t == n_live else above_model.cut_for_total(s, dead, t)
            got = idx.search_batch_above(q[:1], [cut], limit)[0]
            _assert_path(1, 0)
            exp = above_model.above(s, dead, cut, limit)
            assert exp[2] == t
            _check(got, exp, (dtype, t, limit))
            assert best not in got[1]
        # after compact(): the same answers in the new numbering
        old = idx.compact()
        assert idx.n == n_live and old.tolist() == np.nonzero(~dead)[0].tolist()
        s2 = idx.scores(q[0])
        assert s2.view(np.uint32).tolist() == s[old].view(np.uint32).tolist()
        for cut, limit, reruns in ((np.float32(-np.inf), N, 1), (above_model.cut_for_total(s2, None, 700), N, 0)):
            got = idx.search_batch_above(q[:1], [cut], limit)[0]
            _assert_path(1, reruns, rows=n_live)
            _check(got, above_model.above(s2, None, cut, limit), (dtype, "compacted"))
    finally:
        idx.release()


def test_values(case):
    c = case
    s = c.s[0]
    # a cut-off equal to a row's score bits includes that row
    row = int(np.argsort(s)[-40])
    lst, total = c.idx.search_above(c.q[0], float(s[row]), N)
    assert total == 40 and lst[-1] == (float(s[row]), row)
    # -0.0 and +0.0 are one cut-off; +inf admits nothing
    a = c.idx.search_batch_above(c.q[:1], [np.float32(0.0)], 10)[0]
    b = c.idx.search_batch_above(c.q[:1], [np.float32(-0.0)], 10)[0]
    exp = above_model.above(s, None, np.float32(0.0), 10)
    _check(a, exp, "+0.0")
    _check(b, exp, "-0.0")
    assert SORT_CAP < exp[2] <= CAND_CAP              # (about half the rows: the radix-select branch)
    assert c.idx.search_above(c.q[0], float("inf"), 10) == ([], 0)
    with pytest.raises(ValueError, match="query 0"):
        c.idx.search_above(c.q[0], float("nan"), 10)


def test_identical_rows_and_nan_score(gpu, data):
    m, q = data
    m = m[:9001].copy()
    m[8000] = m[17]                         # identical rows: equal score bits, the larger row first
    for dtype in DTYPES:
        mm = m.copy()
        if dtype != "fp8":                  # (an fp8 row's scale is its maximum: whatever that stores, the model follows)
            mm[1234, 5] = np.nan
        idx = svs_amd.DeviceIndex(mm, dtype=dtype)
        try:
            s = idx.scores(q[0])
            assert s[8000].view(np.uint32) == s[17].view(np.uint32)
            got = idx.search_batch_above(q[:1], [s[17]], 9001)[0]
            _check(got, above_model.above(s, None, s[17], 9001), dtype)
            at = got[1].tolist().index(8000)
            assert got[1][at + 1] == 17 and at + 2 == got[2]
            if dtype != "fp8":              # the NaN score qualifies for every cut-off and comes first
                assert np.isnan(s[1234])
                for cut in (np.float32(np.inf), np.float32(0.9), np.float32(-np.inf)):
                    got = idx.search_batch_above(q[:1], [cut], 9001)[0]
                    _check(got, above_model.above(s, None, cut, 9001), (dtype, float(cut)))
                    assert got[1][0] == 1234 and np.isnan(got[0][0])
                assert idx.search_above(q[0], float("inf"), 5)[1] == 1
        finally:
            idx.release()


def test_result_does_not_depend_on_nq(case):
    c = case
    ts = [0, 100, 5000, 33000, 257]         # (33000: a list overflow, re-run with k = 50)
    cuts = [above_model.cut_for_total(c.s[i], None, t) if t else np.float32(np.inf) for i, t in enumerate(ts)]
    batch = c.idx.search_batch_above(c.q, cuts, 50)
    _assert_path(5, 1)
    for i, t in enumerate(ts):
        one = c.idx.search_batch_above(c.q[i:i + 1], cuts[i:i + 1], 50)[0]
        exp = above_model.above(c.s[i], None, cuts[i], 50)
        assert exp[2] == t
        _check(one, exp, (c.dtype, i))
        _check(batch[i], exp, (c.dtype, i, "batch"))
    rev = c.idx.search_batch_above(c.q[::-1], cuts[::-1], 50)[::-1]
    for a, b in zip(rev, batch):
        _check(a, (b[1], b[0], b[2]), "reversed")


def test_against_f64(case):
    c = case
    tol = TOL[c.dtype]
    truth = c.idx.stored_rows().astype(np.float64) @ c.idx.stored_query(c.q[1]).astype(np.float64)
    order = np.sort(truth)[::-1]
    # a cut-off midway between two well-separated scores: the widest gap among ranks 200 .. 400
    gaps = order[200:400] - order[201:401]
    g = 200 + int(np.argmax(gaps))
    cut = np.float32((order[g] + order[g + 1]) / 2)
    assert gaps.max() > 8 * tol
    s, r, total = c.idx.search_batch_above(c.q[1:2], [cut], N)[0]
    print(f"{c.dtype}: cut {float(cut):.7f} total {total} max |score - f64| {np.abs(s - truth[r]).max():.3g}")
    inside = np.abs(truth - float(cut)) <= tol
    assert inside.sum() <= 0.01 * (g + 1)                          # the condition on the inputs
    assert (np.abs(truth[r] - float(cut)) <= tol).sum() <= 0.01 * max(len(r), 1)
    must = np.nonzero(truth >= float(cut) + tol)[0]
    assert np.isin(must, r).all()
    assert (truth[r] >= float(cut) - tol).all()
    assert np.abs(s.astype(np.float64) - truth[r]).max() <= tol
    assert total == len(r)


def test_errors_leave_the_outputs_untouched(case):
    c = case
    limit = 8

    def fresh():
        return (np.full((2, limit), -7.0, dtype=np.float32), np.full((2, limit), -7, dtype=np.int64),
                np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int64))

    def untouched(bufs):
        return all((b == -7).all() for b in bufs)

    q2 = c.q[:2]
    ok = [0.1, 0.2]
    b = fresh()
    assert _raw(c.idx, np.zeros((2, D + 1), dtype=np.float32), ok, limit, *b) == _native.SVS_ERR_SHAPE and untouched(b)
    b = fresh()
    assert _raw(c.idx, q2, [0.1, np.nan], limit, *b) == _native.SVS_ERR_INVALID and untouched(b)
    assert "query 1" in _native.last_error()
    b = fresh()
    assert _raw(c.idx, q2, ok, limit, b[0], b[1], None, b[3]) == _native.SVS_ERR_INVALID and untouched(b)
    b = fresh()
    assert _raw(c.idx, q2, ok, limit, *b, nq=-1) == _native.SVS_ERR_INVALID and untouched(b)
    b = fresh()
    assert _raw(c.idx, q2, ok, limit, None, b[1], b[2], b[3]) == _native.SVS_ERR_INVALID and untouched(b)
    # nq == 0: fine, nothing launched, nothing written
    b = fresh()
    assert _raw(c.idx, q2, ok, limit, *b, nq=0) == 0 and untouched(b) and _native.last_launches() == []


N_DOCS, DIM = 300, 256
BARE = (7, 123, 250)
GONE = tuple(range(40, 60)) + (0, 199, 299)


def _table():
    vecs = _unit(np.random.default_rng(2025), N_DOCS + 2, DIM)
    t = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(N_DOCS)}
    t["ask 0"], t["ask 1"] = ([float(x) for x in vecs[N_DOCS + j]] for j in range(2))
    return t


TABLE = _table()


async def _ef(texts):
    return [TABLE[t] for t in texts]


def test_python_mirror_and_kb(gpu, tmp_path, case):
    c = case
    # DeviceIndex.search_above: python floats and ints, the list search() gives cut by score
    cut = float(above_model.cut_for_total(c.s[2], None, 64))
    lst, total = c.idx.search_above(c.q[2], cut, 1000)
    assert total == 64 and lst == c.idx.search(c.q[2], 64) and isinstance(lst[0][0], float) and isinstance(lst[0][1], int)
    with pytest.raises(ValueError):
        c.idx.search_above(c.q[2][:-1], cut, 5)
    # a small on-disk KB: docs without an embedding, tombstoned rows, embedding ids with gaps
    kb = svs_amd.KB(str(tmp_path / "above.sqlite"), _ef, dtype=c.dtype)
    with kb.bulk_add_docs() as add_doc:
        for i in range(N_DOCS):
            add_doc(f"doc {i}", no_embedding=i in BARE)
    kb.load()
    with kb.bulk_del_docs() as del_doc:
        for i in GONE:
            del_doc(i + 1)
    live = N_DOCS - len(BARE) - len(GONE)
    assert kb.embeddings_matrix.index.n_masked == len(GONE)
    full = kb.retrieve("ask 0", live)
    assert len(full) == live
    cut = full[24]["score"]
    got, total = kb.retrieve_above("ask 0", cut, 10)
    assert total == 25 and [(r["score"], r["doc"]["id"]) for r in got] == [(r["score"], r["doc"]["id"]) for r in full[:10]]
    got, total = kb.retrieve_above("ask 0", cut, 1000)
    assert total == 25 and got == full[:25]
    assert kb.retrieve_above("ask 1", -np.inf, 0) == ([], live)
    # the mirror: embedding ids
    vec = np.array(TABLE["ask 0"], dtype=np.float32)
    ids, total = kb.embeddings_matrix.search_above(vec, cut, 1000)
    assert total == 25 and ids == kb.embeddings_matrix.search(vec, 25)
    with pytest.raises(ValueError):
        kb.retrieve_above("ask 0", float("nan"), 3)
    kb.close()


def test_searches_while_rows_are_appended(gpu, data):
    m, q = data
    m = m[:40000]
    truth = m.astype(np.float64) @ q[0].astype(np.float64)
    cut = float(np.sort(truth)[-150])
    idx = svs_amd.DeviceIndex(m[:20000])
    results, errors = [], []

    def searcher():
        try:
            for _ in range(12):
                results.append(idx.search_above(q[0], cut, 400))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def appender():
        try:
            for r0 in range(20000, 40000, 2000):
                idx.append(m[r0:r0 + 2000])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=searcher) for _ in range(4)] + [threading.Thread(target=appender)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        assert idx.n == 40000 and len(results) == 48
        for lst, total in results:
            rows = np.array([r for _, r in lst], dtype=np.int64)
            sc = np.array([s for s, _ in lst], dtype=np.float64)
            assert total == len(lst) and (rows < 40000).all() and (rows >= 0).all()
            assert np.abs(sc - truth[rows]).max() <= TOL["f32"]
            assert (np.diff(sc) <= 0).all()
            # consistent with SOME prefix of the final matrix: every row below the largest returned one that is clearly
            # above the cut-off was returned
            if len(rows):
                must = np.nonzero(truth[:rows.max()] >= cut + TOL["f32"])[0]
                assert np.isin(must, rows).all()
        final, total = idx.search_above(q[0], cut, 400)
        assert total >= 149 and max(t for _, t in results) <= total
    finally:
        idx.release()

"""GPU: diverse (MMR) search (svs_index_search_diverse; svs_amd/csrc/diverse.h) against its definition.

Candidates and their score bits are what ``idx.search_batch`` returns at fetch_k for the same query batch; the stored
candidate rows come from ``idx.stored_rows``; the picks are judged by ``diverse_model.valid_picks`` (f64, derived
tolerances).  Data: 4,099 rows (no multiple of 4) of 64 unit-norm Gaussian elements, 5 queries; a batch of 17 queries
repeats the 5 cyclically (17 sends the candidate search down a batched route, and equal queries must get equal answers).

Teeth: in one case at most 5 % of the steps may have a second candidate within ``tol`` of the best -- otherwise the
check could not tell answers apart and the case fails."""
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import diverse_model as dm
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, D = 4099, 64
DTYPES = ["f32", "f16", "fp8"]
SHAPES = [(2, 2), (33, 10), (64, 64), (65, 10), (257, 40), (1024, 100)]
LAMS = [0.3, 0.5, 0.9]
NQS = [1, 3, 17]


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    v = v / np.linalg.norm(v, axis=1, keepdims=True)     # (normalised in f64, then cast)
    return v.astype(np.float32)


def _batch(q, nq):
    return np.ascontiguousarray(q[np.arange(nq) % len(q)])


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20261)
    return _unit(rng, N, D), _unit(rng, 5, D)


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    m, q = data
    idx = svs_amd.DeviceIndex(m, dtype=request.param)
    stored = idx.stored_rows()
    stored.setflags(write=False)
    cands = {}      # (nq, fetch_k) -> the candidate search's (scores, rows): computed once, never written

    def candidates(nq, fetch_k):
        if (nq, fetch_k) not in cands:
            s, r = idx.search_batch(_batch(q, nq), fetch_k)
            s.setflags(write=False)
            r.setflags(write=False)
            cands[(nq, fetch_k)] = (s, r)
        return cands[(nq, fetch_k)]

    yield SimpleNamespace(idx=idx, m=m, q=q, stored=stored, candidates=candidates, dtype=request.param)
    idx.release()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def _names():
    return [k for k, _, _ in _native.last_launches()]


def _judge(got, cs, cr, stored, k, lam, d, what, row_offset=0):
    """Every query of one call against its candidates; returns (steps, steps with a second candidate within tol)."""
    s, r, red = got
    nq, c = cs.shape
    count = min(k, c)
    assert s.shape == r.shape == red.shape == (nq, count), (what, s.shape)
    steps = near = 0
    for i in range(nq):
        pos = {int(row): p for p, row in enumerate(cr[i])}
        assert len(set(r[i].tolist())) == count, (what, i, "a row twice")
        assert all(int(row) in pos for row in r[i]), (what, i, "a row that is no candidate")
        picks = [pos[int(row)] for row in r[i]]
        assert _bits(s[i]) == _bits(cs[i][picks]), (what, i, "score bits")
        assert red[i, 0] == -np.inf, (what, i)
        near += dm.valid_picks(cs[i], stored[cr[i] - row_offset], picks, red[i], lam, d)
        steps += count - 1
    return steps, near


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("fetch_k,k", SHAPES)
def test_validity(case, fetch_k, k, lam, nq):
    c = case
    cs, cr = c.candidates(nq, fetch_k)
    got = c.idx.search_batch_diverse(_batch(c.q, nq), k, fetch_k, lam)
    names = _names()
    assert "diverse_gram_kernel" in names and "diverse_pick_kernel" in names, names
    steps, near = _judge(got, cs, cr, c.stored, k, lam, D, (c.dtype, fetch_k, k, lam, nq))
    print(f"{c.dtype} fetch_k={fetch_k} k={k} lam={lam} nq={nq}: {near} of {steps} steps within tol")
    assert near <= 0.05 * steps, f"{near} of {steps} steps have a second candidate within tol: the check has no teeth here"
    # equal queries of a batch get equal answers (nothing depends on the position in the batch)
    for i in range(len(c.q), nq):
        j = i % len(c.q)
        assert got[1][i].tolist() == got[1][j].tolist() and _bits(got[2][i]) == _bits(got[2][j]), (i, j)
    if k > 2 and fetch_k >= 33:
        # a build that ignores G returns the candidates in order
        assert got[1][0].tolist() != cr[0][:k].tolist()


@pytest.mark.parametrize("nq", [1, 17])
@pytest.mark.parametrize("fetch_k,k", [(33, 10), (257, 40), (1024, 100)])
def test_lambda_one_is_the_plain_search(case, fetch_k, k, nq):
    c = case
    qs = _batch(c.q, nq)
    s, r, red = c.idx.search_batch_diverse(qs, k, fetch_k, 1.0)
    es, er = c.idx.search_batch(qs, k)
    cs, cr = c.candidates(nq, fetch_k)
    assert r.tolist() == er.tolist() == cr[:, :k].tolist()
    assert _bits(s) == _bits(es)


def test_one_result_or_one_candidate_launches_nothing_more(case):
    c = case
    qs = _batch(c.q, 3)
    for k, fetch_k in ((1, 1), (1, 40)):      # (one candidate with k > 1: test_single_row_index)
        es, er = c.candidates(3, fetch_k)
        s, r, red = c.idx.search_batch_diverse(qs, k, fetch_k, 0.5)
        assert not [n for n in _names() if n.startswith("diverse_")], _names()
        assert r.tolist() == er[:, :1].tolist() and _bits(s) == _bits(es[:, :1]) and (red == -np.inf).all()
    s, r, red = c.idx.search_batch_diverse(qs, 2, 2, 0.5)
    assert [n for n in _names() if n.startswith("diverse_")] == ["diverse_gram_kernel", "diverse_pick_kernel"]


def test_single_row_index(gpu):
    m = _unit(np.random.default_rng(3), 1, D)
    idx = svs_amd.DeviceIndex(m)
    got = idx.search_diverse(m[0], 5, 8, 0.5)
    assert not [n for n in _names() if n.startswith("diverse_")]
    assert len(got) == 1 and got[0][1] == 0 and got[0][2] == -np.inf and got[0][0] == idx.search(m[0], 1)[0][0]
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_copies_tie_to_the_highest_row(gpu, data, dtype):
    m, q = data
    sc = m.astype(np.float64) @ q[0].astype(np.float64)
    best = np.argsort(-sc)[:8]
    corpus = np.concatenate([m, m[best], m[best]])          # each of the 8 best rows is stored three times
    groups = {int(b): {int(b), N + j, N + 8 + j} for j, b in enumerate(best)}
    top_copy = {row: max(g) for g in groups.values() for row in g}
    idx = svs_amd.DeviceIndex(corpus, dtype=dtype)
    try:
        cs, cr = idx.search_batch(q[:1], 32)
        got = idx.search_batch_diverse(q[:1], 8, 32, 0.5)
        # (exact copies are exact ties BY CONSTRUCTION: a step that picks a copied row always has its copies within tol,
        #  so the teeth condition does not apply here; the tie rule below is what this case pins)
        _judge(got, cs, cr, idx.stored_rows(), 8, 0.5, D, (dtype, "copies"))
        picked = got[1][0].tolist()
        assert any(r in top_copy for r in picked)
        for r in picked:
            if r in top_copy:
                assert r == top_copy[r], f"row {r} was picked, its copy {top_copy[r]} has the higher row number"
    finally:
        idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,fetch_k,k", [(1000, 200, 100, 20), (2000, 1536, 129, 30), (50, 64, 64, 60)])
def test_edges(gpu, dtype, n, d, fetch_k, k):
    # Rows and queries near an 8-dimensional subspace: scores and similarities spread over tenths, as in a real corpus.
    # (Isotropic rows of 1,536 elements are all alike to 0.03, and tol grows with d: 1e-4 there -- a twelfth of the
    #  steps would have a second candidate within it, and the check would have no teeth.)
    rng = np.random.default_rng(n + d)
    basis = rng.standard_normal((8, d))
    m = _unit(rng, n, 8) @ basis + 0.02 * rng.standard_normal((n, d))
    q = _unit(rng, 2, 8) @ basis
    m = (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        cs, cr = idx.search_batch(q, fetch_k)
        got = idx.search_batch_diverse(q, k, fetch_k, 0.5)
        assert got[0].shape == (2, min(k, n, fetch_k))
        steps, near = _judge(got, cs, cr, idx.stored_rows(), k, 0.5, d, (dtype, n, d))
        # (printed, not bounded: tol grows with d -- 9e-5 at d = 1,536 -- and a few steps of 58 do have a second candidate
        #  within it, 1 to 4 depending on the dtype; the 5 % rule belongs to test_validity's data.  Everywhere else
        #  valid_picks forces the f64 arg-max, and a build that ignores G returns the candidates in order.)
        print(f"{dtype} n={n} d={d}: {near} of {steps} steps within tol")
        assert got[1][0].tolist() != cr[0][:got[1].shape[1]].tolist()
    finally:
        idx.release()


def test_masked_rows_and_compaction(gpu, data):
    m, q = data
    idx = svs_amd.DeviceIndex(m[:1500].copy())
    try:
        dead = idx.search_batch(q[:1], 20)[1][0]
        idx.mask_rows(dead)
        cs, cr = idx.search_batch(q[:2], 64)
        got = idx.search_batch_diverse(q[:2], 16, 64, 0.5)
        assert not set(dead.tolist()) & set(got[1].ravel().tolist())
        _judge(got, cs, cr, idx.stored_rows(), 16, 0.5, D, "masked")
        old = idx.compact()                                   # old global row of every new row
        after = idx.search_batch_diverse(q[:2], 16, 64, 0.5)
        assert old[after[1]].tolist() == got[1].tolist()
        assert _bits(after[0]) == _bits(got[0]) and _bits(after[2]) == _bits(got[2])
    finally:
        idx.release()


def _raw(idx, q, k, fetch_k, lam, out_s, out_r, out_red, count, nq=None, d=None, null_q=False):
    q = np.ascontiguousarray(q, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data    # noqa: E731
    return idx._lib.svs_index_search_diverse(idx._handle(), None if null_q else q.ctypes.data, q.shape[0] if nq is None else nq,
                                             q.shape[1] if d is None else d, k, fetch_k, lam, p(out_s), p(out_r), p(out_red),
                                             None if count is None else count.ctypes.data_as(C.POINTER(C.c_int32)))


def test_errors_and_untouched_outputs(case):
    c = case
    q = c.q[:2]
    K = 8

    def fresh():
        return (np.full((2, K), 777.0, np.float32), np.full((2, K), -7, np.int64), np.full((2, K), 555.0, np.float32),
                np.full(1, -99, np.int32))

    def untouched(o):
        return (o[0] == 777.0).all() and (o[1] == -7).all() and (o[2] == 555.0).all() and o[3][0] == -99

    INV, SHP, UNS = _native.SVS_ERR_INVALID, _native.SVS_ERR_SHAPE, _native.SVS_ERR_UNSUPPORTED
    bad = [
        (SHP, dict(k=K, fetch_k=32, lam=0.5, d=D - 1)),
        (INV, dict(k=K, fetch_k=32, lam=0.5, nq=-1)),
        (INV, dict(k=K, fetch_k=32, lam=0.5, null_q=True)),
        (INV, dict(k=K, fetch_k=32, lam=float("nan"))),
        (INV, dict(k=K, fetch_k=32, lam=-0.01)),
        (INV, dict(k=K, fetch_k=32, lam=1.01)),
        (INV, dict(k=K, fetch_k=K - 1, lam=0.5)),
        (INV, dict(k=K, fetch_k=0, lam=0.5)),
        (INV, dict(k=K, fetch_k=-3, lam=0.5)),
        (UNS, dict(k=K, fetch_k=1025, lam=0.5)),
    ]
    for code, kw in bad:
        o = fresh()
        assert _raw(c.idx, q, kw.pop("k"), kw.pop("fetch_k"), kw.pop("lam"), *o, **kw) == code, (code, kw, _native.last_error())
        assert untouched(o), kw
        assert _names() == []
    for missing in range(3):      # out_scores, out_rows, out_count (out_redundancy may be null)
        o = list(fresh())
        o[(0, 1, 3)[missing]] = None
        assert _raw(c.idx, q, K, 32, 0.5, *o) == INV
        assert all((a is None) or (a == b).all() for a, b in zip(o, fresh()))
    empty = svs_amd.DeviceIndex(np.zeros((0, D), np.float32))
    o = fresh()
    assert _raw(empty, q, K, 32, 0.5, *o) == SHP and untouched(o)
    empty.release()
    # k <= 0 and nq == 0: OK, count 0, nothing launched, nothing else written
    for kw in (dict(k=0, fetch_k=32), dict(k=-2, fetch_k=0), dict(k=K, fetch_k=32, nq=0)):
        o = fresh()
        assert _raw(c.idx, q, kw.pop("k"), kw.pop("fetch_k"), 0.5, *o, **kw) == _native.SVS_OK
        assert o[3][0] == (0 if "nq" not in kw else min(K, N)) and (o[0] == 777.0).all() and (o[1] == -7).all() and (o[2] == 555.0).all()
        assert _names() == []
    # success: entries past the count stay untouched; a null out_redundancy is accepted
    small = svs_amd.DeviceIndex(c.m[:5].copy(), dtype=c.dtype)
    o = fresh()
    assert _raw(small, q, K, 32, 0.5, *o) == _native.SVS_OK and o[3][0] == 5
    assert (o[0][:, 5:] == 777.0).all() and (o[1][:, 5:] == -7).all() and (o[2][:, 5:] == 555.0).all()
    assert (o[1][:, :5] >= 0).all() and sorted(o[1][0, :5].tolist()) == [0, 1, 2, 3, 4]
    o2 = list(fresh())
    o2[2] = None
    assert _raw(small, q, K, 32, 0.5, *o2) == _native.SVS_OK
    assert o2[1].tolist() == o[1].tolist() and _bits(o2[0]) == _bits(o[0])
    small.release()


def test_non_finite_data_returns_distinct_candidates(gpu):
    rng = np.random.default_rng(9)
    m = _unit(rng, 300, D)
    m[5, 3] = np.inf
    m[17, 0] = np.nan
    m[40, :] = -np.inf
    idx = svs_amd.DeviceIndex(m)
    try:
        s, r, red = idx.search_batch_diverse(_unit(rng, 2, D), 50, 128, 0.5)
        assert r.shape == (2, 50)
        for i in range(2):
            assert len(set(r[i].tolist())) == 50 and ((0 <= r[i]) & (r[i] < 300)).all()
    finally:
        idx.release()


def test_reentrant_on_one_handle(case):
    c = case
    jobs = [(1, 10, 33), (3, 40, 257), (17, 10, 65), (1, 100, 1024)]
    want = [c.idx.search_batch_diverse(_batch(c.q, nq), k, fk, 0.5) for nq, k, fk in jobs]
    got = [None] * len(jobs)
    errs = []

    def run(i):
        try:
            nq, k, fk = jobs[i]
            for _ in range(3):
                got[i] = c.idx.search_batch_diverse(_batch(c.q, nq), k, fk, 0.5)
                assert got[i][1].tolist() == want[i][1].tolist()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=run, args=(i,)) for i in range(len(jobs))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for g, w in zip(got, want):
        assert g[1].tolist() == w[1].tolist() and _bits(g[0]) == _bits(w[0]) and _bits(g[2]) == _bits(w[2])

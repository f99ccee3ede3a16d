"""GPU: nearest-vector assignment (svs_index_assign; svs_amd/csrc/assign.h) against its definition.

The stored rows come from ``idx.stored_rows``, the stored vectors from a second index of the same dtype built from the
vectors (the ingest path svs_index_debug_query uses); an answer is judged by ``assign_model.valid_assignment`` (f64,
derived tolerances).  Data: 4,099 rows (no multiple of 4 or 64) of unit-norm Gaussian elements, d = 64 and d = 100
(ragged chunks and padding in f16 / fp8), and a pool of 1,024 unit-norm Gaussian vectors of which a case takes the
first c.

Teeth: at most 1 % of the rows of a case may have a second position within ``tol`` of the best -- otherwise the check
could not tell answers apart and the case fails.  (The f64 truth over the f32-cast and over the half-rounded operands of this seed has at
most 3 such rows of 4,099 in every (d, c) below; every case prints its own figure over the stored values.)"""
from types import SimpleNamespace

import numpy as np
import pytest

import assign_model as am
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N = 4099
DIMS = [64, 100]
DTYPES = ["f32", "f16", "fp8"]
CS = [1, 2, 63, 64, 65, 257, 1024]
SEED = 20262
RANGES = [(1, 4097), (4037, 62), (64, 64), (2050, 1)]      # (row0, nrows): [1, 4098), [4037, 4099), [64, 128), one row


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    v = v / np.linalg.norm(v, axis=1, keepdims=True)     # (normalised in f64, then cast)
    return v.astype(np.float32)


def _data(d):
    rng = np.random.default_rng(SEED + d)
    return _unit(rng, N, d), _unit(rng, 1024, d)


def _stored(vectors, dtype):
    """The vectors as stored rows of an index of ``dtype``."""
    tmp = svs_amd.DeviceIndex(vectors, dtype=dtype)
    try:
        return tmp.stored_rows()
    finally:
        tmp.release()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _names():
    return [k for k, _, _ in _native.last_launches()]


@pytest.fixture(scope="module", params=[(d, dt) for d in DIMS for dt in DTYPES], ids=lambda p: f"d{p[0]}-{p[1]}")
def case(request, gpu):
    d, dtype = request.param
    m, pool = _data(d)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    stored = idx.stored_rows()
    stored.setflags(write=False)
    vstored = _stored(pool, dtype)
    vstored.setflags(write=False)
    full = {}      # c -> the full-range answer over pool[:c]: computed once, never written

    def answer(c):
        if c not in full:
            best, sc, counts = idx.assign(pool[:c])
            for a in (best, sc, counts):
                a.setflags(write=False)
            full[c] = (best, sc, counts)
        return full[c]

    yield SimpleNamespace(idx=idx, m=m, pool=pool, stored=stored, vstored=vstored, answer=answer, d=d, dtype=dtype)
    idx.release()


@pytest.mark.parametrize("c", CS)
def test_validity(case, c):
    k = case
    best, sc, counts = k.idx.assign(k.pool[:c])
    names = _names()
    assert names == ["assign_rows_kernel"], names
    assert best.dtype == np.int32 and sc.dtype == np.float32 and counts.dtype == np.int64
    assert best.shape == sc.shape == (N,) and counts.shape == (c,)
    near = am.valid_assignment(k.stored, k.vstored[:c], best, sc, counts, d=k.d)
    print(f"{k.dtype} d={k.d} c={c}: {near} of {N} rows with a second position within tol")
    assert near <= 0.01 * N, f"{near} of {N} rows have a second position within tol: the check has no teeth here"
    assert counts.sum() == N
    if c >= 2:
        assert len(set(best.tolist())) > 1, "every row went to one position: the data is ignored"
    # scores=False: the same positions and counts
    b2, s2, c2 = k.idx.assign(k.pool[:c], scores=False)
    assert s2 is None and np.array_equal(b2, best) and np.array_equal(c2, counts)


def test_planted_rows_find_their_own_vector(case):
    k = case
    rows = sorted({0, N - 1, 63, 64, 65, 127, 128, 4031, 4032, 4095, 4096} | set(np.linspace(200, 3900, 21).astype(int).tolist()))
    assert len(rows) == 32
    c = 40
    V = k.pool[:c].copy()
    slots = np.random.default_rng(3).permutation(c)[:32]
    V[slots] = k.m[rows]          # the rows' own f32 source: ingested as the rows were, so stored alike
    best, sc, counts = k.idx.assign(V)
    assert best[rows].tolist() == slots.tolist()
    e_a, _ = am.tolerances(k.stored, _stored(V, k.dtype), k.d)
    self_dot = (k.stored[rows].astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(sc[rows].astype(np.float64) - self_dot).max() <= e_a


@pytest.mark.parametrize("c", [9, 65, 300])
def test_exact_ties_go_to_the_lower_position(case, c):
    k = case
    V = k.pool[:c].copy()
    V[7] = V[3]
    V[c - 1] = V[0]
    best, sc, counts = k.idx.assign(V)
    assert not (best == 7).any() and not (best == c - 1).any()
    assert counts[7] == 0 and counts[c - 1] == 0 and counts.sum() == N
    assert counts[3] > 0 and counts[0] > 0
    # and the rest is the answer without the copies
    ref, rsc, _ = k.answer(c)
    # (a row whose best was 7 or c - 1 moved elsewhere; every other row keeps its position and its score bits: the copies
    #  only tie with positions 3 and 0, and lose)
    keep = ~np.isin(ref, [7, c - 1])
    assert np.array_equal(best[keep], ref[keep]) and np.array_equal(_bits(sc[keep]), _bits(rsc[keep]))


@pytest.mark.parametrize("c", [5, 257])
def test_answer_depends_only_on_values(case, c):
    k = case
    best, sc, counts = k.answer(c)
    # two identical calls return identical bytes
    b2, s2, c2 = k.idx.assign(k.pool[:c])
    assert b2.tobytes() == best.tobytes() and s2.tobytes() == sc.tobytes() and c2.tobytes() == counts.tobytes()
    # a sub-range: the same positions and score bits row by row, and the counts of those rows
    for row0, nrows in RANGES:
        b, s, cn = k.idx.assign(k.pool[:c], row0=row0, nrows=nrows)
        assert b.shape == (nrows,), (row0, nrows)
        assert np.array_equal(b, best[row0:row0 + nrows]), (row0, nrows)
        assert np.array_equal(_bits(s), _bits(sc[row0:row0 + nrows])), (row0, nrows)
        assert np.array_equal(cn, np.bincount(b, minlength=c)), (row0, nrows)
    # permuted vectors: every row's score BITS unchanged; the position follows the permutation wherever the f64 margin
    # exceeds tol
    perm = np.random.default_rng(c).permutation(c)
    bp, sp, cp = k.idx.assign(k.pool[:c][perm])
    assert np.array_equal(_bits(sp), _bits(sc))
    _, tol = am.tolerances(k.stored, k.vstored[:c], k.d)
    clear = am.margins(k.stored, k.vstored[:c]) > tol
    assert clear.sum() >= 0.99 * N
    assert np.array_equal(perm[bp][clear], best[clear])
    if clear.all():
        assert np.array_equal(cp, counts[perm])
    # A[r][j] does not depend on c or on the sweep width: a row whose best is position 0 scores, against vector 0
    # alone, the same bits
    _, s1, _ = k.answer(1)
    hit = best == 0
    assert hit.any() and np.array_equal(_bits(s1[hit]), _bits(sc[hit]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_tombstones_leave_the_counts_only(gpu, dtype):
    m, pool = _data(64)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        V = pool[:65]
        best, sc, counts = idx.assign(V)
        dead = np.zeros(N, dtype=bool)
        dead[np.random.default_rng(9).choice(N, N // 10, replace=False)] = True
        dead[[0, N - 1]] = True
        idx.mask_rows(np.flatnonzero(dead))
        b2, s2, c2 = idx.assign(V)
        assert b2.tobytes() == best.tobytes() and s2.tobytes() == sc.tobytes()
        assert np.array_equal(c2, np.bincount(best[~dead], minlength=65)) and c2.sum() == N - dead.sum()
        assert np.array_equal(counts - c2, np.bincount(best[dead], minlength=65))
        b3, s3, c3 = idx.assign(V, row0=4037, nrows=62)
        assert np.array_equal(b3, best[4037:]) and c3.sum() == 62 - dead[4037:].sum()
        assert np.array_equal(c3, np.bincount(best[4037:][~dead[4037:]], minlength=65))
    finally:
        idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_label_column_write(gpu, dtype):
    m, pool = _data(100)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        c = 65
        V = pool[:c]
        labels = (np.arange(c, dtype=np.uint32) * 3 + 11)          # distinct, none of them 0
        before = idx.hbm_bytes
        best, sc, counts = idx.assign(V)
        idx._refresh()
        assert idx.hbm_bytes == before and not idx.labels().any()      # no labels: no column
        # the first labelled call allocates the column; labels outside the range stay zero
        b1, s1, c1 = idx.assign(V, labels=labels, row0=64, nrows=1000)
        assert idx.hbm_bytes > before
        grown = idx.hbm_bytes
        col = idx.labels()
        assert np.array_equal(b1, best[64:1064]) and np.array_equal(col[64:1064], labels[best[64:1064]])
        assert not col[:64].any() and not col[1064:].any()
        # a sentinel everywhere, then a sub-range: untouched outside, labels[best] inside
        idx.set_labels(np.full(N, 0xDEAD, dtype=np.uint32))
        idx.assign(V, labels=labels, row0=1, nrows=4097, scores=False)
        col = idx.labels()
        assert col[0] == 0xDEAD and col[N - 1] == 0xDEAD and np.array_equal(col[1:N - 1], labels[best[1:N - 1]])
        # tombstoned rows are labelled too
        idx.mask_rows([5, 70, 4098])
        b2, _, c2 = idx.assign(V, labels=labels)
        assert idx.hbm_bytes == grown and np.array_equal(b2, best) and c2.sum() == N - 3
        col = idx.labels()
        assert np.array_equal(col, labels[best])
        # the labelled search over one topic is the filtered search over that topic's rows, bit for bit
        live = np.ones(N, dtype=bool)
        live[[5, 70, 4098]] = False
        q = pool[200:203]
        order = np.argsort(c2)
        empty = np.flatnonzero(c2 == 0)
        picks = [int(order[-1]), int(order[len(order) // 2])]
        if empty.size:
            picks.append(int(empty[0]))
        else:      # no position without a row: a label no vector carries stands for the topic with count 0
            picks.append(-1)
        for j in picks:
            lab = 7 if j < 0 else int(labels[j])
            rows = np.flatnonzero((best == j) & live) if j >= 0 else np.zeros(0, dtype=np.int64)
            s, r, matched = idx.search_batch_labeled(q, 10, [lab])
            es, er = idx.search_batch_within(q, 10, rows)
            assert matched == len(rows) == (c2[j] if j >= 0 else 0), (j, matched, len(rows))
            assert s.tobytes() == es.tobytes() and np.array_equal(r, er), j
        # appended rows carry label 0
        idx.append(pool[300:310])
        assert idx.n == N + 10 and not idx.labels(N, 10).any() and np.array_equal(idx.labels(0, N), labels[best])
    finally:
        idx.release()


def test_row_offset_is_global(case):
    k = case
    off = svs_amd.DeviceIndex(k.m, dtype=k.dtype, row_offset=1000)
    try:
        c = 65
        best, sc, counts = k.answer(c)
        b, s, cn = off.assign(k.pool[:c])
        assert b.tobytes() == best.tobytes() and s.tobytes() == sc.tobytes() and cn.tobytes() == counts.tobytes()
        b, s, cn = off.assign(k.pool[:c], row0=1064, nrows=64)
        assert np.array_equal(b, best[64:128]) and np.array_equal(_bits(s), _bits(sc[64:128]))
        labels = np.arange(c, dtype=np.uint32) + 1
        off.assign(k.pool[:c], labels=labels, row0=1064, nrows=64)
        col = off.labels()
        assert np.array_equal(col[64:128], labels[best[64:128]]) and not col[:64].any() and not col[128:].any()
        for row0, nrows in ((999, 2), (0, 1), (1000 + N, 1), (1000 + N - 1, 2), (64, 64)):
            with pytest.raises(ValueError):
                off.assign(k.pool[:c], row0=row0, nrows=nrows)
    finally:
        off.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_leave_everything_untouched(gpu, dtype):
    m, pool = _data(64)
    idx = svs_amd.DeviceIndex(m[:300], dtype=dtype)
    lib = _native.load()
    try:
        before = idx.hbm_bytes
        V = np.ascontiguousarray(pool[:4])
        best = np.full(300, -7, dtype=np.int32)
        sc = np.full(300, -7.0, dtype=np.float32)
        cnt = np.full(1100, -7, dtype=np.int64)
        lab = np.arange(1100, dtype=np.uint32) + 1
        big = np.ascontiguousarray(pool[np.arange(1025) % 1024])

        def call(vec, c, d, row0, nrows, labels=lab):
            return lib.svs_index_assign(idx._handle(), None if vec is None else vec.ctypes.data, c, d, row0, nrows,
                                        None if labels is None else labels.ctypes.data, best.ctypes.data, sc.ctypes.data, cnt.ctypes.data)

        for what, args, status in (("c = 0", (V, 0, 64, 0, 300), _native.SVS_ERR_INVALID),
                                   ("c < 0", (V, -1, 64, 0, 300), _native.SVS_ERR_INVALID),
                                   ("c = 1025", (big, 1025, 64, 0, 300), _native.SVS_ERR_UNSUPPORTED),
                                   ("wrong d", (V, 4, 63, 0, 300), _native.SVS_ERR_SHAPE),
                                   ("nrows < 0", (V, 4, 64, 0, -1), _native.SVS_ERR_INVALID),
                                   ("range past the end", (V, 4, 64, 1, 300), _native.SVS_ERR_INVALID),
                                   ("range before the start", (V, 4, 64, -1, 10), _native.SVS_ERR_INVALID),
                                   ("range outside", (V, 4, 64, 301, 1), _native.SVS_ERR_INVALID),
                                   ("null vectors", (None, 4, 64, 0, 300), _native.SVS_ERR_INVALID)):
            assert call(*args) == status, what
            assert _native.last_error(), what
            assert (best == -7).all() and (sc == -7.0).all() and (cnt == -7).all(), what
            idx._refresh()
            assert idx.hbm_bytes == before and not idx.labels().any(), what
            assert _native.last_launches() == [], what
        # the Python layer: the exceptions of the sibling methods
        with pytest.raises(ValueError):
            idx.assign(np.zeros((0, 64), dtype=np.float32))
        with pytest.raises(NotImplementedError):
            idx.assign(big)
        with pytest.raises(ValueError):
            idx.assign(pool[:4, :63])
        with pytest.raises(ValueError):
            idx.assign(pool[0])
        with pytest.raises(ValueError):
            idx.assign(pool[:4], row0=290, nrows=11)
        with pytest.raises(ValueError, match="3 labels for 4 vectors"):
            idx.assign(pool[:4], labels=[1, 2, 3])
        with pytest.raises(ValueError):
            idx.assign(pool[:4], labels=[1, 2, 3, -1])
        idx._refresh()
        assert idx.hbm_bytes == before and not idx.labels().any()
        # nrows == 0: OK, the counts zeroed, nothing launched, no column
        assert call(V, 4, 64, 0, 0) == _native.SVS_OK
        assert (cnt[:4] == 0).all() and (cnt[4:] == -7).all() and (best == -7).all() and _native.last_launches() == []
        b, s, cn = idx.assign(pool[:4], labels=[1, 2, 3, 4], row0=17, nrows=0)
        assert b.shape == (0,) and cn.tolist() == [0, 0, 0, 0] and idx.hbm_bytes == before
        # nothing asked for: OK, nothing launched
        assert lib.svs_index_assign(idx._handle(), V.ctypes.data, 4, 64, 0, 300, None, None, None, None) == _native.SVS_OK
        assert _native.last_launches() == []
        # and the handle still answers
        b, s, cn = idx.assign(pool[:4])
        assert cn.sum() == 300 and _names() == ["assign_rows_kernel"]
    finally:
        idx.release()


def test_nan_scores_win_and_come_back_as_the_quiet_nan(gpu):
    m, pool = _data(64)
    idx = svs_amd.DeviceIndex(m, dtype="f32")
    try:
        for c, bad, want in ((9, [5], 5), (300, [280], 280), (300, [280, 41], 41), (65, [64, 0], 0)):
            V = pool[:c].copy()
            for j in bad:
                V[j, 17] = np.nan
            best, sc, counts = idx.assign(V)
            assert (best == want).all(), (c, bad)
            assert (_bits(sc) == 0x7FC00000).all(), (c, bad)
            assert counts[want] == N and counts.sum() == N
    finally:
        idx.release()

"""GPU: combined search (svs_index_search_combined; svs_amd/csrc/combine.h) against its definition.

The truth is the numpy model (combine_model.py) fed with ``idx.scores(v_j)`` (svs_index_scores_n: the kernel the
definition names): rows, score bits and counts must be EQUAL, on the fused route and on the m-passes route.  A NaN is
compared as THE quiet NaN (key_score's, as in test_above_gpu.py).

Shapes: 2,051 rows (no multiple of 4 or 64; several workgroups for every R x WPB of the one-shot kernels) of unit-norm
Gaussian data; per dtype one d per template family of the fused kernels plus the row lengths that fall back."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import combine_model
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, M_MAX = 2051, 8
# (dtype, d, the fused kernel of that row length or None)
SHAPES = [
    ("f32", 256, "combine_f32_kernel<1, 4, 16>"), ("f32", 768, "combine_f32_kernel<3, 2, 16>"),
    ("f32", 1536, "combine_f32_kernel<6, 1, 16>"), ("f32", 2048, "combine_f32_kernel<8, 1, 8>"),
    ("f32", 4096, "combine_f32_kernel<16, 1, 8>"), ("f32", 100, None), ("f32", 3, None),
    ("f16", 512, "combine_f16_kernel<1, 4, 16>"), ("f16", 1536, "combine_f16_kernel<3, 2, 16>"),
    ("f16", 2048, "combine_f16_kernel<4, 1, 16>"), ("f16", 4096, "combine_f16_kernel<8, 1, 8>"),
    ("f16", 256, None), ("f16", 100, None),
    ("fp8", 512, "combine_fp8_kernel<1, 8, 4, 16>"), ("fp8", 1024, "combine_fp8_kernel<1, 16, 4, 16>"),
    ("fp8", 1536, "combine_fp8_kernel<3, 8, 2, 16>"), ("fp8", 2048, "combine_fp8_kernel<2, 16, 2, 16>"),
    ("fp8", 3072, "combine_fp8_kernel<3, 16, 1, 16>"), ("fp8", 4096, "combine_fp8_kernel<4, 16, 1, 16>"),
    ("fp8", 100, None),
    # rows padded beyond d that still take a fused kernel: the vectors are staged zero padded
    ("f32", 250, "combine_f32_kernel<1, 4, 16>"), ("f16", 500, "combine_f16_kernel<1, 4, 16>"), ("fp8", 1000, "combine_fp8_kernel<1, 16, 4, 16>"),
]
OPS = {"max": 0, "min": 1, "sum": 2}
# a negative, a zero and non-dyadic values: under "sum" a multiplication contracted into the addition rounds differently
MIXED = np.array([0.3, -1.0, 0.0, 0.7, -0.3, 1.5, 0.1, -0.9], dtype=np.float32)
FUSED, PASSES = 1, 2


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _canon(a):
    a = np.asarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _make(dtype, d, n=N, seed=0, edit=None, **kw):
    rng = np.random.default_rng(20270 + d + seed)
    m, v = _unit(rng, n, d), _unit(rng, M_MAX, d)
    if edit:
        edit(m)
    idx = svs_amd.DeviceIndex(m, dtype=dtype, **kw)
    s = [idx.scores(x) for x in v]          # the reference, computed once, never written
    for x in s:
        x.setflags(write=False)
    return SimpleNamespace(idx=idx, v=v, s=s, dtype=dtype, d=d, n=n)


def _hook(idx, vectors, weights, op, route):
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    out = np.empty(len(idx), dtype=np.float32)
    rc = idx._lib.svs_internal_combined_scores(idx._handle(), v.ctypes.data, v.shape[0], v.shape[1], None if w is None else w.ctypes.data,
                                               OPS[op], route, out.ctypes.data, out.size)
    return rc, out


def _expect(c, m, w, op, k, dead=None, row_offset=0):
    return combine_model.top_k(c.s[:m], None if w is None else w[:m], op, k, dead, row_offset)


def _check_topk(got, exp, what):
    s, r, count = got
    eb, er, ecount = exp
    assert count == ecount, (what, count, ecount)
    assert np.asarray(r).tolist() == er[:ecount].tolist(), what
    assert _canon(s).tolist() == eb[:ecount].tolist(), what


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"{p[0]}-{p[1]}")
def shape(request, gpu):
    dtype, d, fused = request.param
    c = _make(dtype, d)
    c.fused = fused
    yield c
    c.idx.release()


def test_whole_vector_on_every_route(shape):
    """Every op, m = 1, 2, 3, 8, with and without weights: the unmasked combined vector of all n rows, from the fused
    kernel (where the row length has one) and from the m passes, equals the model bit for bit."""
    c = shape
    for op in OPS:
        for m in (1, 2, 3, 8):
            for w in (None, MIXED[:m]):
                exp = _canon(combine_model.combine(c.s[:m], w, op))
                for route in (FUSED, PASSES):
                    rc, got = _hook(c.idx, c.v[:m], w, op, route)
                    if route == FUSED and c.fused is None:
                        assert rc == _native.SVS_ERR_UNSUPPORTED, (op, m, rc)
                        continue
                    assert rc == 0, _native.last_error()
                    bad = np.flatnonzero(_canon(got) != exp)
                    assert bad.size == 0, (c.dtype, c.d, op, m, w is not None, route, bad[:5], got[bad[:5]], exp[bad[:5]].view(np.float32))
                    names = [k for k, _, _ in _native.last_launches()]
                    assert (names == [c.fused]) if route == FUSED else (names.count("gemv") == m and names[-1] == "combine_scores_kernel"), names


def test_which_kernel_ran(shape):
    """A public call takes the route's choice.  From two vectors on, where the row length has a fused kernel: that kernel
    once, with (n, m), and no single-query pass.  Elsewhere, and for ONE vector (where the fused kernel was not measured
    faster than the pass, profiles/combined_time.txt): m single-query passes and one combine_scores_kernel."""
    c = shape
    for m in (1, 2, 4, 8):
        s, r, count = c.idx.search_batch_combined(c.v[None, :m], 10, "max")
        rec = _native.last_launches()
        if c.fused and m >= 2:
            assert rec == [(c.fused, N, m)], rec
        else:
            assert [e for e in rec if e[0] == "gemv"] == [("gemv", N, 1)] * m, rec
            assert [e for e in rec if e[0].startswith("combine")] == [("combine_scores_kernel", N, m)], rec
            assert len(rec) == 2 * m + 1 and rec[-1][0] == "combine_scores_kernel", rec
        _check_topk((s[0], r[0], count), _expect(c, m, None, "max", 10), (c.dtype, c.d, m))


# ---- the public entry: one fused and one fallback row length per dtype ------------------------------------------------
PUBLIC = [("f32", 512), ("f32", 100), ("f16", 512), ("f16", 100), ("fp8", 512), ("fp8", 100)]


def _twins(m):
    m[1500] = m[7]          # two identical rows


@pytest.fixture(scope="module", params=PUBLIC, ids=lambda p: f"{p[0]}-{p[1]}")
def pub(request, gpu):
    c = _make(*request.param, seed=1, edit=_twins)
    yield c
    c.idx.release()


def _raw(idx, vectors, weights, op, k, out_s, out_r, count, nq=None, m=None, d=None):
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    return idx._lib.svs_index_search_combined(idx._handle(), p(v), v.shape[0] if nq is None else nq, v.shape[1] if m is None else m,
                                              v.shape[2] if d is None else d, p(w), op, k, p(out_s), p(out_r),
                                              None if count is None else C.byref(count))


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("k", [1, 10, N, N + 5])
def test_top_k(pub, op, k):
    """k = 1, 10, n and n + 5: the C entry writes count = min(k, n) entries and touches nothing behind them."""
    c = pub
    out_s = np.full((1, k), 123.0, dtype=np.float32)
    out_r = np.full((1, k), -77, dtype=np.int64)
    count = C.c_int32(-1)
    assert _raw(c.idx, c.v[None, :3], MIXED[None, :3], OPS[op], k, out_s, out_r, count) == 0, _native.last_error()
    exp = _expect(c, 3, MIXED, op, k)
    cnt = count.value
    assert cnt == min(k, N)
    _check_topk((out_s[0, :cnt], out_r[0, :cnt], cnt), exp, (c.dtype, c.d, op, k))
    assert (out_s[0, cnt:] == 123.0).all() and (out_r[0, cnt:] == -77).all()
    # the wrapper: clamped to the live rows, the same answer
    s, r, n_out = c.idx.search_batch_combined(c.v[None, :3], k, op, MIXED[None, :3])
    assert s.shape == r.shape == (1, cnt)
    _check_topk((s[0], r[0], n_out), exp, (c.dtype, c.d, op, k, "wrapper"))


def test_one_vector_max_is_search(pub):
    c = pub
    s, r, count = c.idx.search_batch_combined(c.v[:4, None, :], 50, "max")
    assert count == 50
    for q in range(4):      # (one query per call: the single-query kernel, the one the definition names)
        es, er = c.idx.search_batch(c.v[q:q + 1], 50)
        assert r[q].tolist() == er[0].tolist() and _canon(s[q]).tolist() == _canon(es[0]).tolist()
    assert c.idx.search_combined(c.v[:1], 50) == c.idx.search(c.v[0], 50)


def test_three_queries_in_one_call_equal_three_calls(pub):
    c = pub
    vec = np.stack([c.v[0:3], c.v[2:5], c.v[5:8]])
    w = np.stack([MIXED[0:3], MIXED[2:5], MIXED[5:8]])
    for op in OPS:
        s, r, count = c.idx.search_batch_combined(vec, 20, op, w)
        for q in range(3):
            s1, r1, c1 = c.idx.search_batch_combined(vec[q:q + 1], 20, op, w[q:q + 1])
            assert c1 == count == 20 and r[q].tolist() == r1[0].tolist() and _canon(s[q]).tolist() == _canon(s1[0]).tolist()
        _check_topk((s[1], r[1], count), combine_model.top_k(c.s[2:5], MIXED[2:5], op, 20), (c.dtype, op))


def test_identical_rows_tie_by_row(pub):
    """Rows 7 and 1,500 are one vector: equal combined scores, adjacent in the answer, in the order of the top-k stage."""
    c = pub
    for op in OPS:
        s, r, count = c.idx.search_batch_combined(c.v[None, :3], N, op)
        _check_topk((s[0], r[0], count), _expect(c, 3, None, op, N), (c.dtype, op))
        rows = r[0].tolist()
        i, j = rows.index(7), rows.index(1500)
        assert abs(i - j) == 1 and s[0][i].view(np.uint32) == s[0][j].view(np.uint32)


def test_row_offset_and_tombstones(gpu):
    """row_offset is added to every row; the best row of the combined order and ten others are masked: none comes back
    and count = min(k, live)."""
    for dtype, d in (("f32", 512), ("fp8", 100)):
        c = _make(dtype, d, seed=2, row_offset=1000)
        try:
            for op in OPS:
                _check_topk(_first(c.idx.search_batch_combined(c.v[None, :3], 10, op, MIXED[None, :3])),
                            _expect(c, 3, MIXED, op, 10, None, 1000), (dtype, op, "offset"))
            best = _expect(c, 3, MIXED, "sum", 1, None, 0)[1][0]
            dead = np.unique(np.concatenate([[best], np.arange(40, 2040, 200)])).astype(np.int64)
            assert dead.size == 11
            c.idx.mask_rows(dead + 1000)
            for op in OPS:
                for k in (10, N):
                    got = _first(c.idx.search_batch_combined(c.v[None, :3], k, op, MIXED[None, :3]))
                    assert got[2] == min(k, N - 11) and not set(got[1].tolist()) & set((dead + 1000).tolist())
                    _check_topk(got, _expect(c, 3, MIXED, op, k, dead, 1000), (dtype, op, k, "masked"))
        finally:
            c.idx.release()


def _first(res):
    s, r, count = res
    return s[0], r[0], count


def test_window_selection_path(gpu):
    """40,003 x 512 f16, k = 100: the window path of the top-k stage over the combined vector."""
    c = _make("f16", 512, n=40003, seed=3)
    try:
        for op in OPS:
            got = _first(c.idx.search_batch_combined(c.v[None, :4], 100, op, MIXED[None, :4]))
            assert _native.last_launches() == [("combine_f16_kernel<1, 4, 16>", 40003, 4)]
            _check_topk(got, _expect(c, 4, MIXED, op, 100), op)
    finally:
        c.idx.release()


@pytest.mark.parametrize("dtype,d", [("f32", 256), ("f32", 100), ("f16", 512), ("f16", 100)])
def test_special_values(gpu, dtype, d):
    """A stored row with a NaN element scores NaN against every vector: it ranks first under every op (under "min" because
    EVERY term is NaN).  An all-zero row under a negative weight has the term -0: it compares, and comes back, as +0."""
    def edit(m):
        m[11, 5] = np.nan
        m[300] = 0.0
    c = _make(dtype, d, seed=4, edit=edit)
    try:
        assert all(np.isnan(s[11]) for s in c.s) and all(s[300] == 0 for s in c.s)
        w = np.array([-1.0, 0.5, -0.25], dtype=np.float32)
        for op in OPS:
            exp = _canon(combine_model.combine(c.s[:3], w, op))
            for route in (FUSED, PASSES):
                rc, got = _hook(c.idx, c.v[:3], w, op, route)
                if rc == _native.SVS_ERR_UNSUPPORTED and route == FUSED and d == 100:
                    continue
                assert rc == 0 and (_canon(got) == exp).all(), (dtype, d, op, route)
                assert np.isnan(got[11])
            got = _first(c.idx.search_batch_combined(c.v[None, :3], 5, op, w[None]))
            _check_topk(got, _expect(c, 3, w, op, 5), (dtype, d, op))
            assert got[1][0] == 11 and np.isnan(got[0][0])
        # the zero row: one vector, weight -1 -> the term is -0; max / min fold it onto +0
        for op in ("max", "min"):
            rc, got = _hook(c.idx, c.v[:1], np.array([-1.0], dtype=np.float32), op, PASSES)
            assert rc == 0 and got[300].view(np.uint32) == 0
        # a NaN term among finite ones: "min" is NaN only where every term is -- row 11 here, no other row
        rc, got = _hook(c.idx, c.v[:3], None, "min", PASSES)
        assert rc == 0 and np.flatnonzero(np.isnan(got)).tolist() == [11]
    finally:
        c.idx.release()


def test_screened_index_answers_from_its_f32_rows(gpu):
    """An f32 index of 32,768 x 512 with the half shadow kept and screening forced on: a combined search reads the f32
    rows (svs_index_scores_n's kernel), never the shadow."""
    c = _make("f32", 512, n=32768, seed=5)
    try:
        c.idx.set_screen(1)
        c.idx.set_variant(12)
        assert c.idx.screen_stats()["shadow"] == 1
        for op in OPS:
            got = _first(c.idx.search_batch_combined(c.v[None, :3], 100, op, MIXED[None, :3]))
            assert _native.last_launches() == [("combine_f32_kernel<2, 4, 16>", 32768, 3)]
            _check_topk(got, _expect(c, 3, MIXED, op, 100), op)
        s, r, _ = c.idx.search_batch_combined(c.v[None, :1], 100, "max")
        assert _canon(s[0]).tolist() == combine_model.top_k(c.s[:1], None, "max", 100)[0].tolist()
    finally:
        c.idx.release()


def test_errors(pub):
    c = pub
    idx, v = c.idx, c.v[None, :2]
    out_s, out_r, count = np.zeros((1, 4), dtype=np.float32), np.zeros((1, 4), dtype=np.int64), C.c_int32(0)
    INVALID = _native.SVS_ERR_INVALID

    def bad(rc, text):
        assert rc == INVALID, (rc, text)
        assert text in _native.last_error(), (text, _native.last_error())

    bad(idx._lib.svs_index_search_combined(None, v.ctypes.data, 1, 2, c.d, None, 0, 4, out_s.ctypes.data, out_r.ctypes.data, C.byref(count)), "null index")
    bad(_raw(idx, v, None, 0, 4, out_s, out_r, count, nq=-1), "nq")
    bad(_raw(idx, v, None, 0, 4, out_s, out_r, count, m=0), "m is 0")
    bad(_raw(idx, v, None, 0, 4, out_s, out_r, count, m=9), "m is 9")
    bad(_raw(idx, v, None, 0, 4, out_s, out_r, count, d=c.d + 1), "d is")
    bad(_raw(idx, v, None, 3, 4, out_s, out_r, count), "op")
    bad(_raw(idx, v, None, -1, 4, out_s, out_r, count), "op")
    bad(_raw(idx, v, None, 0, -1, out_s, out_r, count), "k must")
    bad(idx._lib.svs_index_search_combined(idx._handle(), None, 1, 2, c.d, None, 0, 4, out_s.ctypes.data, out_r.ctypes.data, C.byref(count)), "null vectors")
    bad(_raw(idx, v, None, 0, 4, None, out_r, count), "null output")
    bad(_raw(idx, v, None, 0, 4, out_s, None, count), "null output")
    for w in (np.nan, np.inf, -np.inf):
        bad(_raw(idx, v, np.array([[1.0, w]], dtype=np.float32), 2, 4, out_s, out_r, count), "vector 1 of query 0")
    assert (out_s == 0).all() and (out_r == 0).all()          # a failing call writes no output
    # nq == 0 and k == 0: SVS_OK, nothing launched; null outputs are fine with nothing to write
    assert _raw(idx, v, None, 0, 4, None, None, count, nq=0) == 0 and _native.last_launches() == []
    assert _raw(idx, v, None, 0, 0, None, None, count) == 0 and count.value == 0 and _native.last_launches() == []
    # the wrapper's own checks
    for call in (lambda: idx.search_batch_combined(c.v[:2], 4), lambda: idx.search_batch_combined(np.zeros((1, 9, c.d), np.float32), 4),
                 lambda: idx.search_batch_combined(np.zeros((1, 0, c.d), np.float32), 4), lambda: idx.search_batch_combined(v, 4, "mean"),
                 lambda: idx.search_batch_combined(v, 4, "sum", [1.0, 2.0]), lambda: idx.search_batch_combined(v, 4, "sum", [[1.0, np.nan]]),
                 lambda: idx.search_batch_combined(np.zeros((1, 2, c.d + 1), np.float32), 4), lambda: idx.search_combined(v, 4),
                 lambda: idx.search_combined(c.v[:2], 4, "sum", [[1.0, 2.0]])):
        with pytest.raises(ValueError):
            call()

"""GPU: the group-combined search (svs_index_search_collapsed_combined; svs_amd/csrc/collapse_combine.h and the
multi-score kernels of combine.h) against its definition.

The truth is ``idx.scores(v_j)`` per vector (svs_index_scores_n: the single-query kernel), ``idx.column(c)`` and the
masked rows fed to the numpy model (collapsed_combined_model.py): rows, values, counts and groups must be EQUAL, score
bits equal (the model returns them as every search does: -0.0 as +0.0, a NaN as 0x7fc00000).  No tolerances.

Shape A: N = 24,579 rows (24 strips of 1,024 rows + 3) of 64 unit-norm Gaussian elements under f32, f16 and fp8 -- no
fused kernel at this row length, so the score pass is m single-query passes -- with 8 vectors, of which m = 1, 2, 3, 8
are used.  Row 17 (strip 0) IS vector 0 and row 20000 (strip 19) IS vector 1: the two facet-covering chunks of one
parent wherever a test puts them under one value.  Shape B: 2,051 x 512, which has a fused multi-score kernel in all
three dtypes, m = 2 and 8.  One more case has more strips than the kernels' grid cap has workgroups (d = 16).

Columns 1 and 2 are written by the tests as they need them; column 3 is NEVER set by any test of this file."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import collapse_model
import combine_model
import svs_amd
from collapsed_combined_model import collapsed_combined
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, D = 24579, 64
NB, DB = 2051, 512
DTYPES = ["f32", "f16", "fp8"]
MS = [1, 2, 3, 8]
OPS = ["max", "min", "sum"]
NEVER_SET = 3
SINGLE, GROUP = "single", "group"
# a negative, a zero and non-dyadic values: under "sum" a multiplication contracted into the addition rounds differently
MIXED = np.array([1.0, -0.7, 0.3, 1.9, 0.0, -1.1, 0.45, 2.3], dtype=np.float32)
POSITIVE = np.array([1.0, 0.7, 0.3, 1.9, 0.0, 1.1, 0.45, 2.3], dtype=np.float32)
FUSED = {("f32", 512): "multi_score_f32_kernel<2, 4, 16>", ("f16", 512): "multi_score_f16_kernel<1, 4, 16>",
         ("fp8", 512): "multi_score_fp8_kernel<1, 8, 4, 16>"}


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _make(n, d, seed):
    rng = np.random.default_rng(seed)
    m = _unit(rng.standard_normal((n, d)))
    v = _unit(rng.standard_normal((8, d)))
    m[17] = v[0]
    m[min(20000, n - 40)] = v[1]
    m.setflags(write=False)
    return m, v


@pytest.fixture(scope="module")
def data():
    return _make(N, D, 20264)


def _case(m, v, dtype):
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    s = [idx.scores(x) for x in v]            # the reference, computed once, never written
    for x in s:
        x.setflags(write=False)
    return SimpleNamespace(idx=idx, s=s, m=m, v=v, dtype=dtype, n=len(m))


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    c = _case(*data, request.param)
    yield c
    c.idx.release()


@pytest.fixture(scope="module", params=DTYPES)
def fused(request, gpu):
    c = _case(*_make(NB, DB, 20265), request.param)
    c.kernel = FUSED[(request.param, DB)]
    yield c
    c.idx.release()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


def _check(got, exp, what, row_offset=0):
    s, r, v, g = got
    es, er, ev, eg = exp
    assert g == eg, (what, g, eg)
    assert r.tolist() == (er + row_offset).tolist(), what
    assert v.tolist() == ev.tolist(), what
    assert _bits(s) == _bits(es), what


def _one(idx, vectors, n, column, op, w, zero):
    """One combined query through the Python entry: (scores, rows, values, groups), trimmed to the count."""
    s, r, v, counts, groups = idx.search_batch_collapsed_combined(vectors[None], n, column, op, None if w is None else w[None], zero)
    c = int(counts[0])
    assert c == min(max(n, 0), int(groups[0]), s.shape[1])
    return s[0, :c], r[0, :c], v[0, :c], int(groups[0])


def _ask(c, m, op, w, column, values, zero, n, dead=None, what=None, first=0):
    """Vectors first .. first + m, checked against the model over ``values`` (what the test wrote into ``column``)."""
    sel = slice(first, first + m)
    w = None if w is None else np.ascontiguousarray(w[sel])
    got = _one(c.idx, c.v[sel], n, column, op, w, zero)
    exp = collapsed_combined(c.s[sel], w, op, values, dead, zero == SINGLE, n)
    _check(got, exp, (c.dtype, what, m, op, zero, n))
    return got


def _set(c, column, values):
    values = np.ascontiguousarray(values, dtype=np.uint32)
    c.idx.set_column(column, values)
    assert c.idx.column(column).tolist() == values.tolist()
    return values


def _raw(idx, vectors, weights, op, k, column, zero_mode, outs, counts, groups, nq=None, m=None, d=None):
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    return idx._lib.svs_index_search_collapsed_combined(idx._handle(), v.ctypes.data, v.shape[0] if nq is None else nq,
                                                        v.shape[1] if m is None else m, v.shape[2] if d is None else d, p(weights),
                                                        op, k, column, zero_mode, *[p(o) for o in outs], p(counts), p(groups))


def _fresh(nq, k):
    outs = (np.full((nq, k), -7.0, dtype=np.float32), np.full((nq, k), -7, dtype=np.int64), np.full((nq, k), 7, dtype=np.uint32))
    return outs, np.full(nq, -7, dtype=np.int32), np.full(nq, -7, dtype=np.int64)


def _untouched(outs, counts=None, groups=None, frm=0):
    ok = (outs[0][..., frm:] == -7).all() and (outs[1][..., frm:] == -7).all() and (outs[2][..., frm:] == 7).all()
    return ok and (counts is None or (counts == -7).all()) and (groups is None or (groups == -7).all())


# ---- shape A -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_adjacent_runs(case, m):
    """Runs of 7 rows straddle a thread's four rows, a wave, a strip and a workgroup; runs of 64 and 256 put whole waves
    and workgroups on one slot; runs of 3 put several values into a thread.  Catches errors in the thread's fold of the
    m keys and in the per-vector maxima."""
    c = case
    v = _set(c, 1, np.arange(N) // 7 + 1)
    for op in OPS:
        for w in (None, MIXED):
            for zero in (SINGLE, GROUP):
                got = _ask(c, m, op, w, 1, v, zero, 100, what="runs of 7")
                assert got[3] == (N + 6) // 7 and len(set(got[2].tolist())) == 100
    for run in (64, 256, 3):
        v = _set(c, 1, np.arange(N) // run + 1)
        for op in OPS:
            assert _ask(c, m, op, MIXED, 1, v, SINGLE, 150, what=("runs", run))[3] == (N + run - 1) // run


def test_facets_in_far_apart_strips(case):
    """Rows 17 (strip 0, vector 0 itself) and 20000 (strip 19, vector 1 itself) under ONE value: under "min" that parent
    is first with min(1, 1), represented by one of the two, while the row-level search ranks neither first by that score."""
    c = case
    vals = np.arange(N, dtype=np.uint32) + 1
    vals[20000] = vals[17] = 4_000_000
    v = _set(c, 1, vals)
    for op in OPS:
        sc, r, gv, g = _ask(c, 2, op, None, 1, v, SINGLE, 50, what="facets")
        assert g == N - 1 and gv[0] == 4_000_000 and r[0] in (17, 20000)
    sc, r, gv, g = _ask(c, 2, "min", None, 1, v, SINGLE, 5, what="facets, min")
    both = min(np.float32(c.s[0][17]), np.float32(c.s[1][20000]))
    rs, rr, _ = c.idx.search_batch_combined(c.v[None, :2], 1, "min")
    assert sc[0] == both and both > 0.8 > rs[0, 0]                # no single row covers both facets
    # a second pair, the other way round in row order, plus a third row of the group that wins neither vector
    vals[[5000, 17, 20000]] = 4_000_001
    v = _set(c, 1, vals)
    sc, r, gv, g = _ask(c, 2, "min", None, 1, v, SINGLE, 5, what="three rows")
    assert gv[0] == 4_000_001 and sc[0] == both and g == N - 2


@pytest.mark.parametrize("m", MS)
def test_identity_one_row_per_group_is_the_combined_search(case, m):
    """Identity 2: a column never set under ZERO_SINGLE, every op and weight -- svs_index_search_combined's rows and bits."""
    c = case
    assert not c.idx.column(NEVER_SET).any()
    for op in OPS:
        for w in (None, MIXED):
            for k in (1, 100, 2049):
                sc, r, gv, g = _ask(c, m, op, w, NEVER_SET, None, SINGLE, k, what="never set")
                ps, pr, count = c.idx.search_batch_combined(c.v[None, :m], k, op, None if w is None else w[None, :m])
                assert g == N and count == k and r.tolist() == pr[0].tolist() and _bits(sc) == _bits(ps[0]) and not gv.any()
    # ZERO_IS_GROUP: one group, scored by the best row per vector
    sc, r, gv, g = _ask(c, m, "min", None, NEVER_SET, None, GROUP, 10, what="one group")
    assert g == 1 and sc[0] == min(np.float32(x.max()) for x in c.s[:m])


def test_identity_one_vector_max_is_the_collapsed_search(case):
    """Identity 1: m == 1, no weights, "max" -- svs_index_search_collapsed: rows, values, groups and score bits."""
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    vecs = c.v[[0, 3, 5]]
    for column in (1, NEVER_SET):
        for zero in (SINGLE, GROUP):
            a = c.idx.search_batch_collapsed_combined(vecs[:, None, :], 120, column, "max", None, zero)
            b = c.idx.search_batch_collapsed(vecs, 120, column, zero)
            assert a[3].tolist() == b[3].tolist() and a[4].tolist() == b[4].tolist()
            for qi in range(3):
                cnt = int(a[3][qi])
                assert a[1][qi, :cnt].tolist() == b[1][qi, :cnt].tolist() and a[2][qi, :cnt].tolist() == b[2][qi, :cnt].tolist()
                assert _bits(a[0][qi, :cnt]) == _bits(b[0][qi, :cnt])


@pytest.mark.parametrize("m", [2, 3, 8])
def test_identity_max_with_non_negative_weights_is_collapsing_the_combined_vector(case, m):
    """Identity 3: max over rows and max over vectors commute under a monotone multiplication."""
    c = case
    v = _set(c, 2, (np.arange(N) * 2654435761 % 3001).astype(np.uint32))      # 3,001 scattered groups, 0 among them
    for w in (None, POSITIVE):
        c_row = combine_model.combine(c.s[:m], None if w is None else w[:m], "max")
        for zero in (SINGLE, GROUP):
            got = _ask(c, m, "max", w, 2, v, zero, 200, what="identity 3")
            es, er, ev, eg = collapse_model.collapsed(c_row, v, None, zero == SINGLE, 200)
            assert got[3] == eg and got[1].tolist() == er.tolist() and got[2].tolist() == ev.tolist() and _bits(got[0]) == _bits(es)


def test_sum_with_a_negative_weight(case):
    """"like vector 0, unlike vector 1" per parent: the group's best row for vector 1 counts AGAINST it, whichever row
    that is."""
    c = case
    v = _set(c, 1, np.arange(N) // 7 + 1)
    w = np.array([1.0, -1.0], dtype=np.float32)
    sc, r, gv, g = _ask(c, 2, "sum", np.concatenate([w, MIXED[2:]]), 1, v, SINGLE, 300, what="negative weight")
    grp = 17 // 7 + 1
    rows = np.nonzero(v == grp)[0]
    want = np.float32(np.float32(c.s[0][rows].max()) + np.float32(-1.0) * np.float32(c.s[1][rows].max()))
    i = gv.tolist().index(grp)
    assert sc[i] == want


def test_value_zero_in_both_modes(case):
    c = case
    vals = (np.arange(N) // 7 + 1).astype(np.uint32)
    vals[50:60] = 0
    vals[17] = 0
    v = _set(c, 1, vals)
    others = len(set(vals.tolist())) - 1
    for m in (2, 8):
        for op in OPS:
            assert _ask(c, m, op, MIXED, 1, v, GROUP, N, what="0 is a group")[3] == others + 1
            got = _ask(c, m, op, MIXED, 1, v, SINGLE, N, what="0 stands alone")
            assert got[3] == others + 11 and sorted(got[1][got[2] == 0].tolist()) == [17] + list(range(50, 60))


def test_tombstones(gpu, data, case):
    """A dead representative hands over; a dead row's per-vector maximum no longer counts; a group masked whole is
    absent; a dead row never comes back through its score."""
    m, vec = data
    dtype = case.dtype
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        c = SimpleNamespace(idx=idx, s=case.s, v=vec, dtype=dtype)
        vals = (np.arange(N) // 7 + 1).astype(np.uint32)
        vals[50:60] = 0
        vals[20000] = vals[17]
        v = _set(c, 2, vals)
        dead = np.zeros(N, dtype=bool)
        before = _ask(c, 2, "min", None, 2, v, SINGLE, 40, what="before")
        top_value = int(vals[17])
        assert before[2][0] == top_value
        rep = int(before[1][0])
        dead[rep] = True
        idx.mask_rows([rep])
        after = _ask(c, 2, "min", None, 2, v, SINGLE, N, dead=dead, what="representative masked")
        i = after[2].tolist().index(top_value)
        assert after[3] == before[3] and after[1][i] != rep and vals[after[1][i]] == top_value       # another row stands for it
        dead[17] = True
        idx.mask_rows([17])
        after = _ask(c, 2, "min", None, 2, v, SINGLE, N, dead=dead, what="a facet masked")
        i = after[2].tolist().index(top_value)
        assert after[3] == before[3] and after[0][i] < before[0][0]       # the chunk that answered vector 0 is gone: the parent drops
        members = np.nonzero(vals == top_value)[0]
        dead[members] = True
        idx.mask_rows(members)
        gone = _ask(c, 2, "min", None, 2, v, SINGLE, N, dead=dead, what="group masked")
        assert gone[3] == before[3] - 1 and top_value not in gone[2].tolist()
        # exempt rows die alone; each of the four nibble positions, a whole bitmap word; then a random 5 %
        more = [52, 57, 1000, 1001, 1002, 1003, 2005, 2010, 2015, 2016] + list(range(6400, 6432))
        dead[more] = True
        idx.mask_rows(more)
        for zero in (SINGLE, GROUP):
            _ask(c, 3, "sum", MIXED, 2, v, zero, 500, dead=dead, what="nibbles")
        rnd = np.nonzero((np.random.default_rng(8).random(N) < 0.05) & ~dead)[0]
        dead[rnd] = True
        idx.mask_rows(rnd)
        for mm in MS:
            for op in OPS:
                got = _ask(c, mm, op, MIXED, 2, v, SINGLE, N, dead=dead, what="5 % masked")
                assert not dead[got[1]].any() and len(got[1]) == got[3]
        sc, r, gv, g = _ask(c, 3, "max", None, NEVER_SET, None, SINGLE, 100, dead=dead, what="never set, masked")
        ps, pr, _ = idx.search_batch_combined(vec[None, :3], 100, "max")
        assert g == int((~dead).sum()) and r.tolist() == pr[0].tolist() and _bits(sc) == _bits(ps[0])
    finally:
        idx.release()


def test_counts(case):
    c = case
    v = _set(c, 1, np.arange(N) % 5 + 10)
    vec = c.v[None, :3]
    w = np.ascontiguousarray(MIXED[None, :3])
    exp = collapsed_combined(c.s[:3], w[0], "sum", v, None, True, 100)
    # k larger than the number of groups: count 5, the entries past it hold the caller's sentinel
    for k in (9, 5, 3, 1):
        outs, counts, groups = _fresh(1, k)
        assert _raw(c.idx, vec, w, 2, k, 1, 1, outs, counts, groups) == 0, _native.last_error()
        cnt = min(k, 5)
        assert counts.tolist() == [cnt] and groups.tolist() == [5]
        _check(tuple(o[0, :cnt] for o in outs) + (5,), tuple(e[:cnt] for e in exp[:3]) + (5,), (c.dtype, "k", k))
        assert _untouched(outs, frm=cnt)
    # k = 0 and k < 0: count-only, null result pointers; out_groups may be NULL
    for k in (0, -4):
        counts, groups = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int64)
        assert _raw(c.idx, vec, w, 2, k, 1, 1, (None,) * 3, counts, groups) == 0, _native.last_error()
        assert counts.tolist() == [0] and groups.tolist() == [5]
    counts = np.full(1, -7, dtype=np.int32)
    assert _raw(c.idx, vec, None, 0, 0, 1, 1, (None,) * 3, counts, None) == 0 and counts.tolist() == [0]
    assert _one(c.idx, c.v[:3], 0, 1, "sum", None, SINGLE)[3] == 5
    # nq == 0: nothing launched, nothing written
    outs, counts, groups = _fresh(2, 3)
    assert _raw(c.idx, np.zeros((2, 3, D), np.float32), None, 0, 3, 1, 1, outs, counts, groups, nq=0) == 0
    assert _untouched(outs, counts, groups) and _native.last_launches() == []
    # fewer groups than k on the window and the sorted route of the top-k stage: the struck rows fill the selection, the host trims
    for k in (100, 2049):
        assert len(_ask(c, 2, "min", None, 1, v, GROUP, k, what=("few groups", k))[1]) == 5
    # more groups than k on both
    v = _set(c, 1, np.arange(N) // 3 + 1)
    for k in (1, 257, 2049):
        assert len(_ask(c, 3, "max", MIXED, 1, v, SINGLE, k, what=("route", k))[1]) == k


def test_three_queries_in_one_call_equal_three_calls(case):
    """... and the same call twice, and a call on ANOTHER column or with another m in between: a table or a key array
    not left empty would carry maxima over."""
    c = case
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, (np.arange(N) * 2654435761 % 3001).astype(np.uint32))
    vec = np.stack([c.v[0:3], c.v[2:5], c.v[5:8]])
    w = np.stack([MIXED[0:3], MIXED[2:5], MIXED[5:8]])
    for column, v, op in ((1, v1, "min"), (2, v2, "sum"), (1, v1, "max"), (NEVER_SET, None, "sum"), (2, v2, "min")):
        for zero in (SINGLE, GROUP):
            for _ in range(2):
                s, r, gv, counts, groups = c.idx.search_batch_collapsed_combined(vec, 120, column, op, w, zero)
                for qi, first in enumerate((0, 2, 5)):
                    exp = collapsed_combined(c.s[first:first + 3], w[qi], op, v, None, zero == SINGLE, 120)
                    cnt = int(counts[qi])
                    _check((s[qi, :cnt], r[qi, :cnt], gv[qi, :cnt], int(groups[qi])), exp, (c.dtype, "batch", column, zero, qi))
                    _check(_one(c.idx, vec[qi], 120, column, op, w[qi], zero), exp, (c.dtype, "alone", column, zero, qi))
            _ask(c, 8, op, MIXED, 1, v1, zero, 50, what="m = 8 in between")        # (another key layout on the same context)
            c.idx.search_batch_collapsed(c.v[:1], 10, 2, zero)                    # (the collapsed search shares the table)


def test_all_four_entries_share_the_tables_of_one_context(gpu, data, case):
    """One handle, one thread, so one context: group-combined with m = 8 and m = 2 (two key layouts), the collapsed
    search (the same table, no keys), the collapsed search under a predicate and over a row list of 254 rows (a table of
    the smallest size inside the large one), then group-combined with m = 3.  Every answer equals its model, and each
    group-combined answer equals, byte for byte, the same call on a fresh handle over the same data: a table or a key
    array that one entry left behind would add groups or raise maxima in the next."""
    c = case
    m, vec = data
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, np.arange(N) % 97)
    where = [(2, "in", [5])]
    in_scope = v2 == 5
    rows = np.flatnonzero(in_scope)
    assert len(rows) == 254
    q = c.v[3:5]
    ps, pr = c.idx.search_batch_within(q, len(rows), rows)          # the scope's truth: every row of it once, the gather kernel's bits
    t = np.zeros((2, N), dtype=np.float32)
    for qi in range(2):
        assert sorted(pr[qi].tolist()) == rows.tolist()
        t[qi, pr[qi]] = ps[qi]
    K = 120

    def combined(idx, mm, op):
        out = idx.search_batch_collapsed_combined(c.v[None, :mm], K, 1, op, MIXED[None, :mm], SINGLE)
        cnt = int(out[3][0])
        _check((out[0][0, :cnt], out[1][0, :cnt], out[2][0, :cnt], int(out[4][0])),
               collapsed_combined(c.s[:mm], MIXED[:mm], op, v1, None, True, K), (c.dtype, "shared tables", mm, op))
        return [np.ascontiguousarray(a[0, :cnt]).tobytes() for a in out[:3]] + [out[3].tolist(), out[4].tolist()]

    def scoped(out, what):
        s, r, gv, counts, groups, matched = out
        assert matched == 254
        for qi in range(2):
            es, er, ev, eg = collapse_model.collapsed(t[qi], v1, ~in_scope, True, K)
            cnt = int(counts[qi])
            _check((s[qi, :cnt], r[qi, :cnt], gv[qi, :cnt], int(groups[qi])), (es, er, ev, eg), (c.dtype, what, qi))

    got = [combined(c.idx, 8, "sum"), combined(c.idx, 2, "min")]
    s, r, gv, counts, groups = c.idx.search_batch_collapsed(q, K, 1, SINGLE)
    for qi in range(2):
        cnt = int(counts[qi])
        _check((s[qi, :cnt], r[qi, :cnt], gv[qi, :cnt], int(groups[qi])), collapse_model.collapsed(c.s[3 + qi], v1, None, True, K),
               (c.dtype, "collapsed", qi))
    scoped(c.idx.search_batch_collapsed_where(q, K, where, 1, SINGLE), "where")
    scoped(c.idx.search_batch_collapsed_within(q, K, rows, 1, SINGLE), "rows")
    got.append(combined(c.idx, 3, "max"))
    for (mm, op), answer in zip(((8, "sum"), (2, "min"), (3, "max")), got):
        fresh = svs_amd.DeviceIndex(m, dtype=c.dtype)
        try:
            fresh.set_column(1, v1)
            assert combined(fresh, mm, op) == answer, (c.dtype, "fresh handle", mm, op)
        finally:
            fresh.release()


def test_nan_score_is_the_largest(gpu, data):
    m, vec = data
    mm = m[:9001].copy()
    mm[1234, 5] = np.nan
    idx = svs_amd.DeviceIndex(mm, dtype="f32")
    try:
        s = [idx.scores(x) for x in vec[:3]]
        assert all(np.isnan(x[1234]) for x in s)
        c = SimpleNamespace(idx=idx, s=s, v=vec, dtype="f32")
        v = _set(c, 1, np.arange(9001) // 7 + 1)
        for op in OPS:          # (under "min" too: EVERY per-vector maximum of that group is the NaN)
            sc, r, gv, g = _ask(c, 3, op, MIXED, 1, v, SINGLE, 10, what="nan")
            assert r[0] == 1234 and np.isnan(sc[0]) and gv[0] == 1234 // 7 + 1 and not set(range(1232, 1239)) & set(r[1:].tolist())
    finally:
        idx.release()


def test_row_offset_append_and_compact(gpu, data, case):
    m, vec = data
    dtype = case.dtype
    off = 1_000_000
    idx = svs_amd.DeviceIndex(m[:9000], dtype=dtype, row_offset=off)
    try:
        w = np.ascontiguousarray(MIXED[:3])
        ask = lambda n, zero: _one(idx, vec[:3], n, 1, "sum", w, zero)
        vals = (np.arange(9000) // 6 + 1).astype(np.uint32)
        idx.set_column(1, vals)
        s = [idx.scores(x) for x in vec[:3]]
        got = ask(80, SINGLE)
        _check(got, collapsed_combined(s, w, "sum", vals, None, True, 80), "row_offset", row_offset=off)
        assert (got[1] >= off).all()
        # after append: the new rows carry 0 -- each its own group, or one group; the table and the keys grow with the rows
        idx.append(m[9000:9500])
        s2 = [idx.scores(x) for x in vec[:3]]
        vals2 = np.concatenate([vals, np.zeros(500, dtype=np.uint32)])
        for zero, groups in ((SINGLE, 1500 + 500), (GROUP, 1500 + 1)):
            got = ask(3000, zero)
            _check(got, collapsed_combined(s2, w, "sum", vals2, None, zero == SINGLE, 3000), ("append", zero), row_offset=off)
            assert got[3] == groups
        dead = np.zeros(9500, dtype=bool)
        dead[[0, 55, 123, 4000, 9499]] = True
        dead[2000:2600] = True
        idx.mask_rows(np.nonzero(dead)[0] + off)
        _check(ask(200, SINGLE), collapsed_combined(s2, w, "sum", vals2, dead, True, 200), "masked", row_offset=off)
        idx.compact()
        keep = np.nonzero(~dead)[0]
        s3 = [idx.scores(x) for x in vec[:3]]
        _check(ask(200, SINGLE), collapsed_combined(s3, w, "sum", vals2[keep], None, True, 200), "compacted", row_offset=off)
    finally:
        idx.release()


def test_two_threads_on_one_handle_with_different_columns(case):
    """Each context owns its table and keys: concurrent calls on different columns and with different m must not see
    each other's groups."""
    c = case
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, np.arange(N) % 911)
    asks = [(2, "min", 1, v1, SINGLE), (8, "sum", 2, v2, GROUP), (3, "max", 2, v2, SINGLE), (2, "sum", NEVER_SET, None, SINGLE)]
    want = [collapsed_combined(c.s[:m], MIXED[:m], op, v, None, zero == SINGLE, 150) for m, op, _, v, zero in asks]
    got = [[] for _ in asks]
    errors = []

    def work(i):
        m, op, column, _, zero = asks[i]
        try:
            for _ in range(6):
                got[i].append(_one(c.idx, c.v[:m], 150, column, op, np.ascontiguousarray(MIXED[:m]), zero))
        except BaseException as e:          # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(asks))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, answers in enumerate(got):
        assert len(answers) == 6
        for a in answers:
            _check(a, want[i], (c.dtype, "thread", i))


def test_launch_record(case):
    """The kernels under test ran: per combined query m "gemv" passes with the kernel svs_index_scores_n runs (this row
    length has no fused kernel), then the reduce and the mark kernel."""
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    c.idx.search_batch_collapsed_combined(np.stack([c.v[0:3], c.v[3:6]]), 5, 1, "min")
    rec = _native.last_launches()
    names = [k for k, _, _ in rec]
    assert [e for e in rec if e[0] == "cc_reduce_kernel"] == [("cc_reduce_kernel", N, 3)] * 2
    assert [e for e in rec if e[0] == "cc_mark_kernel"] == [("cc_mark_kernel", N, 3)] * 2
    assert names.count("gemv") == 6 and len(names) == 16, names
    kernels = [k for k in names if k not in ("gemv", "cc_reduce_kernel", "cc_mark_kernel")]
    assert len(kernels) == 6 and len(set(kernels)) == 1, names
    c.idx.scores(c.v[0])
    assert _native.last_launches()[1][0] == kernels[0]
    for i in (0, 8):
        assert names[i:i + 6:2] == ["gemv"] * 3 and names[i + 6:i + 8] == ["cc_reduce_kernel", "cc_mark_kernel"]
    # a count-only call runs them too
    c.idx.search_batch_collapsed_combined(c.v[None, :2], 0, 1, "max")
    assert [k for k, _, _ in _native.last_launches()][4:] == ["cc_reduce_kernel", "cc_mark_kernel"]


def test_argument_errors_leave_the_outputs_untouched(case):
    c = case
    k = 4
    vec = np.stack([c.v[0:2], c.v[2:4]])
    INV = _native.SVS_ERR_INVALID

    def call(expect, *args, outs=True, counts=True, **kw):
        o, cn, g = _fresh(2, k)
        rc = _raw(c.idx, *args, o if outs is True else outs, cn if counts else None, g, **kw)
        assert rc == expect, (rc, _native.last_error())
        assert _untouched(o, cn, g) and _native.last_launches() == []
        assert "svs_index_search_collapsed_combined" in _native.last_error()
        return _native.last_error()

    call(INV, vec, None, 0, k, 1, 1, d=D + 1)
    call(INV, vec, None, 0, k, 1, 1, nq=-1)
    for m in (0, 9, -1):
        call(INV, vec, None, 0, k, 1, 1, m=m)
    for op in (-1, 3):
        assert "op" in call(INV, vec, None, op, k, 1, 1)
    for bad in (np.nan, np.inf):
        w = np.ones((2, 2), dtype=np.float32)
        w[1, 0] = bad
        assert "weight" in call(INV, vec, w, 2, k, 1, 1)
    for column in (-1, 4, 1 << 20):
        assert "column" in call(INV, vec, None, 0, k, column, 1)
    for mode in (-1, 2, 77):
        assert "zero_mode" in call(INV, vec, None, 0, k, 1, mode)
    call(INV, vec, None, 0, k, 1, 1, counts=False)
    for missing in range(3):
        o, cn, g = _fresh(2, k)
        part = tuple(None if i == missing else x for i, x in enumerate(o))
        assert _raw(c.idx, vec, None, 0, k, 1, 1, part, cn, g) == INV and _untouched(o, cn, g)
    o, cn, g = _fresh(2, k)
    assert c.idx._lib.svs_index_search_collapsed_combined(c.idx._handle(), None, 2, 2, D, None, 0, k, 1, 1, *[x.ctypes.data for x in o],
                                                          cn.ctypes.data, g.ctypes.data) == INV
    assert _untouched(o, cn, g)
    for bad in (-1, 4, True, "1"):
        with pytest.raises(ValueError):
            c.idx.search_collapsed_combined(c.v[:2], 3, bad)
    with pytest.raises(ValueError):
        c.idx.search_collapsed_combined(c.v[:2], 3, 1, "max", None, "both")
    with pytest.raises(ValueError):
        c.idx.search_collapsed_combined(c.v[None, :2], 3, 1)
    hits, groups = c.idx.search_collapsed_combined(c.v[:2], 3, NEVER_SET, "min", None, GROUP)
    assert groups == 1 and len(hits) == 1 and hits[0][2] == 0 and isinstance(hits[0][0], float)


# ---- shape B: the fused multi-score kernels --------------------------------------------------------------------------------
def _multi_scores(idx, vectors, route):
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    out = np.full((v.shape[0], len(idx)), np.float32(-7.0), dtype=np.float32)
    rc = idx._lib.svs_internal_multi_scores(idx._handle(), v.ctypes.data, v.shape[0], v.shape[1], route, out.ctypes.data, out.size)
    return rc, out


@pytest.mark.parametrize("m", [2, 8])
def test_multi_score_pass_equals_a_single_query_pass_per_vector(fused, m):
    """The hook on the fused route and on the passes route: bit-equal to idx.scores(v_j) for every j; the record names
    the kernel that ran."""
    c = fused
    for route, first in ((1, 0), (2, 0), (0, 8 - m)):
        rc, out = _multi_scores(c.idx, c.v[first:first + m], route)
        assert rc == 0, _native.last_error()
        rec = _native.last_launches()
        if route == 2:
            assert [k for k, _, _ in rec].count("gemv") == m and len(rec) == 2 * m and not [k for k, _, _ in rec if "multi_score" in k]
        else:
            assert rec == [(c.kernel, NB, m)], rec
        for j in range(m):
            assert _bits(out[j]) == _bits(c.s[first + j]), (c.dtype, route, j)
    # the capacity is checked
    v = np.ascontiguousarray(c.v[:m])
    out = np.zeros(m * NB - 1, dtype=np.float32)
    assert c.idx._lib.svs_internal_multi_scores(c.idx._handle(), v.ctypes.data, m, DB, 0, out.ctypes.data, out.size) == _native.SVS_ERR_INVALID


def test_the_fused_route_needs_a_fused_kernel(case):
    rc, _ = _multi_scores(case.idx, case.v[:2], 1)
    assert rc == _native.SVS_ERR_UNSUPPORTED and "fused" in _native.last_error()
    rc, out = _multi_scores(case.idx, case.v[:2], 0)
    assert rc == 0 and _bits(out[0]) == _bits(case.s[0]) and _bits(out[1]) == _bits(case.s[1])


@pytest.mark.parametrize("m", [2, 8])
def test_public_call_on_the_fused_route(fused, m):
    c = fused
    v = _set(c, 1, np.arange(NB) // 5 + 1)
    for op in OPS:
        for w in (None, MIXED):
            for zero in (SINGLE, GROUP):
                _ask(c, m, op, w, 1, v, zero, 60, what="fused")
        rec = _native.last_launches()
        assert rec == [(c.kernel, NB, m), ("cc_reduce_kernel", NB, m), ("cc_mark_kernel", NB, m)], rec
    got = _ask(c, m, "min", None, NEVER_SET, None, SINGLE, NB, what="fused, never set")
    assert got[3] == NB
    # one query vector (m = 1) takes the single-query pass, as svs_index_search_combined does
    _ask(c, 1, "max", None, 1, v, SINGLE, 20, what="one vector")
    assert [k for k, _, _ in _native.last_launches()][0] == "gemv"


# ---- more strips than workgroups ---------------------------------------------------------------------------------------
def test_several_strips_per_workgroup(gpu):
    """Every workgroup of the capped grid takes two strips, the first a third, and a ragged rest of 3 rows: the strided
    loops of both kernels.  Groups of 5 (the first few of 6) scattered over the whole corpus by r % (n // 5)."""
    geo = np.zeros(2, dtype=np.int32)
    assert _native.load().svs_internal_collapse_geometry(geo.ctypes.data_as(_native.C.POINTER(_native.C.c_int32))) == 0
    strip, grid = int(geo[0]), int(geo[1])
    n = 2 * grid * strip + strip + 3
    d = 16
    rng = np.random.default_rng(79)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    vec = _unit(rng.standard_normal((2, d)))
    vals = (np.arange(n) % (n // 5)).astype(np.uint32)
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    try:
        idx.set_column(1, vals)
        dead = np.zeros(n, dtype=bool)
        dead[rng.integers(0, n, 5000)] = True
        dead[[n - 1, grid * strip, grid * strip + 1]] = True
        idx.mask_rows(np.nonzero(dead)[0])
        s = [idx.scores(x) for x in vec]
        for zero in (GROUP, SINGLE):
            got = _one(idx, vec, 100, 1, "min", None, zero)
            rec = _native.last_launches()
            assert rec[-2:] == [("cc_reduce_kernel", n, 2), ("cc_mark_kernel", n, 2)]
            _check(got, collapsed_combined(s, None, "min", vals, dead, zero == SINGLE, 100), ("strided", zero))
        assert got[3] >= n // 5 - 1
    finally:
        idx.release()

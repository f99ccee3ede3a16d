"""GPU: the scoped collapsed searches (svs_index_search_collapsed_where / _rows; svs_amd/csrc/collapse_scope.h) against
their definition.

The truth of a scope is what the definition names: ``search_batch_where(q, matched, where)`` (for a row list:
``search_batch_within``) returns every row of S once with the gather kernel's score bits; they are scattered into a
length-N vector and fed, with the numpy predicate mask (where_model.where_mask) and the masked rows, to the numpy model
(collapse_scope_model.py).  Rows, values, counts, groups and matched must be EQUAL, score bits equal with NaN
canonicalised.  No tolerances.

Shape: test_collapse_gpu.py's -- N = 24,579 rows (12 filter strips of 2,048 rows + 3, 24 collapse strips of 1,024 + 3,
no multiple of 4) of 64 unit-norm Gaussian elements, under f32, f16 and fp8, 3 queries.  Row N - 1 IS query 0; rows 17
and 20000 are one vector, rows 33 and 15000 another.  The tests write columns 0, 1 and 2 as they need them (``_set``
keeps a host copy for the predicate model); column 3 is NEVER set by any test of this file."""
import ctypes as C
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import collapse_model
import select_cases
import svs_amd
from collapse_scope_model import collapsed_scoped
from svs_amd import _native
from test_where_gpu import PREDICATES, VALUES
from where_model import where_mask

pytestmark = pytest.mark.gpu

N, D = 24579, 64
DTYPES = ["f32", "f16", "fp8"]
NEVER_SET = 3
SINGLE, GROUP = "single", "group"


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(20263)
    m = _unit(rng.standard_normal((N, D)))
    q = _unit(rng.standard_normal((3, D)))
    near = lambda w: _unit(q[0] + w * _unit(rng.standard_normal(D)))
    m[N - 1] = q[0]
    m[17] = m[20000] = near(0.3)
    m[33] = m[15000] = near(0.4)
    m.setflags(write=False)
    return m, q


def _case(m, q, dtype, **kw):
    idx = svs_amd.DeviceIndex(m, dtype=dtype, **kw)
    return SimpleNamespace(idx=idx, m=m, q=q, dtype=dtype, n=len(m), cols={}, dead=np.zeros(len(m), dtype=bool), off=idx.row_offset)


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    c = _case(*data, request.param)
    yield c
    c.idx.release()


def _canon(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).tolist()


def _set(c, column, values):
    values = np.ascontiguousarray(values, dtype=np.uint32)
    c.idx.set_column(column, values)
    c.cols[column] = values
    return values


def _mask(c, rows):
    rows = np.asarray(rows, dtype=np.int64)
    c.idx.mask_rows(rows + c.off)
    c.dead[rows] = True


def _scatter(c, s, r):
    """Every row of S once, with its score: (t (nq, n), the rows of S ascending)."""
    t = np.zeros((len(c.q), c.n), dtype=np.float32)
    for qi in range(len(c.q)):
        assert len(set(r[qi].tolist())) == r.shape[1]
        t[qi, r[qi] - c.off] = s[qi]
    return t, (np.sort(r[0]) - c.off if r.shape[1] else np.zeros(0, dtype=np.int64))


def _truth_where(c, where):
    """(t (nq, n) f32, in_scope bool (n,), matched) of a predicate: the model's mask, checked against the device's S."""
    mask = where_mask(c.cols, where, c.n)
    matched = c.idx.count_where(where)
    s, r, again = c.idx.search_batch_where(c.q, matched, where)
    t, rows = _scatter(c, s, r)
    assert matched == again == r.shape[1] and rows.tolist() == np.flatnonzero(mask & ~c.dead).tolist()
    return t, mask, matched


def _truth_rows(c, rows):
    rows = np.asarray(rows, dtype=np.int64)
    mask = np.zeros(c.n, dtype=bool)
    mask[rows - c.off] = True
    s, r = c.idx.search_batch_within(c.q, len(rows), rows)
    t, got = _scatter(c, s, r)
    assert got.tolist() == np.flatnonzero(mask & ~c.dead).tolist()
    return t, mask, r.shape[1]


def _same(got, exp, what, off=0):
    """got: (scores, rows, values, groups, matched) trimmed to the count; exp: the model's five (local rows)."""
    s, r, v, g, m = got
    es, er, ev, eg, em = exp
    assert (g, m) == (eg, em), (what, g, m, eg, em)
    assert r.tolist() == (er + off).tolist(), what
    assert v.tolist() == ev.tolist(), what
    assert _canon(s) == _canon(es), what


def _trim(out, qi, n):
    s, r, v, counts, groups, matched = out
    cnt = int(counts[qi])
    assert cnt == min(max(n, 0), int(groups[qi]), s.shape[1])
    return s[qi, :cnt], r[qi, :cnt], v[qi, :cnt], int(groups[qi]), matched


def _ask(c, where, column, zero, n, truth=None, what=None, qs=(0, 1, 2)):
    """The batch of three under ``where``, every query checked against the model; returns query qs[0]'s answer."""
    t, mask, matched = truth or _truth_where(c, where)
    out = c.idx.search_batch_collapsed_where(c.q, n, where, column, zero)
    first = None
    for qi in qs:
        exp = collapsed_scoped(t[qi], c.cols.get(column), c.dead, mask, zero == SINGLE, n)
        got = _trim(out, qi, n)
        _same(got, exp, (c.dtype, what, where if len(str(where)) < 80 else "...", zero, n, qi), c.off)
        first = first or got
    return first


def _ask_rows(c, rows, column, zero, n, truth=None, what=None):
    t, mask, matched = truth or _truth_rows(c, rows)
    out = c.idx.search_batch_collapsed_within(c.q, n, rows, column, zero)
    first = None
    for qi in range(3):
        exp = collapsed_scoped(t[qi], c.cols.get(column), c.dead, mask, zero == SINGLE, n)
        got = _trim(out, qi, n)
        _same(got, exp, (c.dtype, what, "rows", zero, n, qi), c.off)
        first = first or got
    return first


ODD = [(0, "in", [1])]


def test_representatives_inside_the_scope(case):
    """Runs of 7 under a scope of the odd rows: m = 12,289 (no multiple of 4), every run straddles the scope.  The best
    row of the corpus, N - 1, is even: its group is represented by its best ODD row, with that row's own score."""
    c = case
    v = _set(c, 1, np.arange(N) // 7 + 1)
    _set(c, 0, np.arange(N) % 2)
    truth = _truth_where(c, ODD)
    assert truth[2] == N // 2 == 12289 and truth[2] % 4
    for zero in (SINGLE, GROUP):
        s, r, gv, g, m = _ask(c, ODD, 1, zero, 100, truth, "odd rows")
        assert g == (N + 6) // 7 and (r % 2 == 1).all() and len(set(gv.tolist())) == 100
    s, r, gv, g, m = _ask(c, ODD, 1, SINGLE, N, truth, "odd rows, every group", qs=(0,))
    assert len(r) == g
    top = int(v[N - 1])
    i = gv.tolist().index(top)
    scoped_row = int(r[i])
    us, ur, uv, _, _ = c.idx.search_batch_collapsed(c.q[:1], 1, 1, SINGLE)
    assert ur[0, 0] == N - 1 and uv[0, 0] == top                  # the unscoped representative ...
    assert scoped_row != N - 1 and scoped_row % 2 == 1 and v[scoped_row] == top
    assert _canon(s[i:i + 1]) == _canon(truth[0][0, scoped_row:scoped_row + 1]) != _canon(us[0, :1])   # ... and the scoped one's own bits
    # a group whose rows are all out of scope is absent: column 2 strikes the whole run of value 101 through a second term
    flag = np.zeros(N, dtype=np.uint32)
    flag[v == 101] = 9
    _set(c, 2, flag)
    where = ODD + [(2, "not in", [9])]
    s, r, gv, g2, m2 = _ask(c, where, 1, SINGLE, N, what="a group out of scope")
    assert g2 == g - 1 and m2 == truth[2] - int(((v == 101) & (np.arange(N) % 2 == 1)).sum()) and 101 not in gv.tolist()


def test_predicate_on_the_grouping_column(case):
    """The write kernel reuses the registers the predicate loaded: three values of 7 rows, m = 21."""
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    where = [(1, "in", [5, 2900, 3511])]
    for zero in (SINGLE, GROUP):
        s, r, gv, g, m = _ask(c, where, 1, zero, 10, what="on the grouping column")
        assert (g, m, len(r)) == (3, 21, 3) and sorted(gv.tolist()) == [5, 2900, 3511]
    # ... and with the value 0 among the three: one group or seven
    _set(c, 1, np.arange(N) // 7)
    where = [(1, "in", [0, 2900, 3510])]
    assert _ask(c, where, 1, SINGLE, 50, what="0 in the set")[3:] == (2 + 7, 21)
    assert _ask(c, where, 1, GROUP, 50, what="0 in the set")[3:] == (3, 21)


def test_scope_sizes_at_the_edges(case):
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    _set(c, 2, np.arange(N))
    n_d = max(n for n in select_cases.D_SIZES if n % 4)
    assert n_d == 4095
    # m = 0: only the count kernel runs
    where = [(2, "range", (N, N + 5))]
    for k in (1, 100, 0):
        s, r, gv, counts, groups, matched = c.idx.search_batch_collapsed_where(c.q, k, where, 1, SINGLE)
        assert matched == 0 and not counts.any() and not groups.any()
        assert [e[0] for e in _native.last_launches()] == ["where_count_kernel"]
    scopes = [("m = 1", (5, 5), 1), ("the ragged tail", (N - 3, N - 1), 3), ("one workgroup selects", (100, 100 + n_d - 1), n_d),
              ("just above", (100, 100 + n_d + 1), n_d + 2)]
    for what, (lo, hi), m in scopes:
        where = [(2, "range", (lo, hi))]
        truth = _truth_where(c, where)
        assert truth[2] == m
        for k in (1, 100, 2049):
            if k > m and k != 1:
                continue
            for zero in (SINGLE, GROUP):
                got = _ask(c, where, 1, zero, k, truth, what)
                assert got[4] == m and got[3] == len(set((np.arange(lo, hi + 1) // 7).tolist()))
        # the whole scope asked for: k = m
        _ask(c, where, NEVER_SET, SINGLE, m, truth, what)
    assert _ask(c, [(2, "range", (N - 3, N - 1))], 1, SINGLE, 5)[1][0] == N - 1


def test_value_zero_and_the_identities(case):
    c = case
    vals = (np.arange(N) // 7 + 1).astype(np.uint32)
    vals[50:60] = 0
    _set(c, 1, vals)
    _set(c, 0, (np.arange(N) % 3 != 0).astype(np.uint32))          # two rows of three in scope
    where = [(0, "in", [1])]
    truth = _truth_where(c, where)
    zeros_in = [r for r in range(50, 60) if r % 3]
    others = len({int(x) for x in vals[(np.arange(N) % 3 != 0)]}) - 1
    s, r, gv, g, m = _ask(c, where, 1, SINGLE, N, truth, "0 stands alone")
    assert g == others + len(zeros_in) and sorted(r[gv == 0].tolist()) == zeros_in
    s, r, gv, g, m = _ask(c, where, 1, GROUP, N, truth, "0 is a group")
    assert g == others + 1 and gv.tolist().count(0) == 1
    # identity (a): a column never set under ZERO_SINGLE is search_batch_where; (b): under ZERO_IS_GROUP its first row
    assert not c.idx.column(NEVER_SET).any()
    for k in (1, 100, 2049):
        ps, pr, pm = c.idx.search_batch_where(c.q, k, where)
        out = c.idx.search_batch_collapsed_where(c.q, k, where, NEVER_SET, SINGLE)
        one = c.idx.search_batch_collapsed_where(c.q, k, where, NEVER_SET, GROUP)
        for qi in range(3):
            s, r, gv, g, m = _trim(out, qi, k)
            assert (g, m) == (pm, pm) and r.tolist() == pr[qi].tolist() and _canon(s) == _canon(ps[qi]) and not gv.any()
            s, r, gv, g, m = _trim(one, qi, k)
            assert (g, m, r.tolist(), gv.tolist()) == (1, pm, pr[qi, :1].tolist(), [0]) and _canon(s) == _canon(ps[qi, :1])
    rows = np.flatnonzero(np.arange(N) % 3 != 0)
    ps, pr = c.idx.search_batch_within(c.q, 100, rows)
    out = c.idx.search_batch_collapsed_within(c.q, 100, rows, NEVER_SET, SINGLE)
    for qi in range(3):
        s, r, gv, g, m = _trim(out, qi, 100)
        assert (g, m) == (len(rows), len(rows)) and r.tolist() == pr[qi].tolist() and _canon(s) == _canon(ps[qi])


def test_ties(case):
    """One vector under ONE value in filter strips 0 and 9: the larger row wins while it is in scope, the smaller one
    when it is not.  One vector under TWO values: both appear, the larger row first."""
    c = case
    vals = np.arange(N, dtype=np.uint32) + 1
    vals[20000] = vals[17]
    _set(c, 1, vals)
    scope = np.ones(N, dtype=np.uint32)
    scope[::7] = 0                                                 # (17, 33, 15000 and 20000 are no multiples of 7)
    _set(c, 0, scope)
    truth = _truth_where(c, ODD)
    t = truth[0][0]
    assert t[17].view(np.uint32) == t[20000].view(np.uint32) and t[33].view(np.uint32) == t[15000].view(np.uint32)
    s, r, gv, g, m = _ask(c, ODD, 1, SINGLE, 60, truth, "both in scope")
    rows = r.tolist()
    assert 20000 in rows and 17 not in rows and gv[rows.index(20000)] == 18
    i = rows.index(15000)
    assert rows[i + 1] == 33 and s[i].view(np.uint32) == s[i + 1].view(np.uint32) and gv[i] != gv[i + 1]
    scope[20000] = 0
    _set(c, 0, scope)
    s, r, gv, g2, m2 = _ask(c, ODD, 1, SINGLE, 60, what="the larger row out of scope")
    rows = r.tolist()
    assert 17 in rows and 20000 not in rows and gv[rows.index(17)] == 18 and (g2, m2) == (g, m - 1)


def test_tombstones(gpu, data, case):
    """A masked representative hands over to the runner-up IN SCOPE; masked rows never count in matched; each of the
    four nibble positions; a random 5 %."""
    c = _case(*data, case.dtype)
    try:
        vals = _set(c, 2, np.arange(N) // 7 + 1)
        _set(c, 0, np.arange(N) % 2)
        before = _ask(c, ODD, 2, SINGLE, 40, what="before")
        top, rep = int(before[2][0]), int(before[1][0])              # query 0's best group in scope and its representative
        assert int(((vals == top) & (np.arange(N) % 2 == 1)).sum()) >= 3
        _mask(c, [rep])
        after = _ask(c, ODD, 2, SINGLE, N, what="representative masked")
        j = after[2].tolist().index(top)
        assert after[3] == before[3] and after[4] == before[4] - 1
        assert after[1][j] != rep and after[1][j] % 2 == 1 and vals[after[1][j]] == top      # the runner-up in scope
        _mask(c, np.flatnonzero((vals == top) & (np.arange(N) % 2 == 1)))                     # the group's even rows stay live
        gone = _ask(c, ODD, 2, SINGLE, N, what="group masked in scope")
        assert top not in gone[2].tolist() and gone[3] == before[3] - 1
        _mask(c, [52, 57, 1000, 1001, 1002, 1003, 2005, 2010, 2015, 2016] + list(range(6400, 6432)))
        for zero in (SINGLE, GROUP):
            _ask(c, ODD, 2, zero, 500, what="nibbles")
        _mask(c, np.flatnonzero((np.random.default_rng(8).random(N) < 0.05) & ~c.dead))
        got = _ask(c, ODD, 2, SINGLE, N, what="5 % masked")
        assert not c.dead[got[1]].any() and got[4] == int((~c.dead[1::2]).sum())
        rows = np.random.default_rng(9).integers(0, N, 5000)
        got = _ask_rows(c, rows, 2, GROUP, 300, what="5 % masked, a row list")
        assert got[4] == int((~c.dead[np.unique(rows)]).sum())
    finally:
        c.idx.release()


def test_nan_in_and_out_of_scope(gpu, data):
    m, q = data
    mm = m[:9001].copy()
    mm[1235, 5] = np.nan
    c = _case(mm, q, "f32")
    try:
        _set(c, 1, np.arange(9001) // 7 + 1)
        _set(c, 0, np.arange(9001) % 2)
        s, r, gv, g, mt = _ask(c, ODD, 1, SINGLE, 10, what="nan in scope")
        assert r[0] == 1235 and np.isnan(s[0]) and gv[0] == 1235 // 7 + 1 and not set(range(1232, 1239)) & set(r[1:].tolist())
        s, r, gv, g, mt = _ask(c, [(0, "in", [0])], 1, SINGLE, 9001, what="nan out of scope")
        assert 1235 not in r.tolist() and not np.isnan(s).any() and 1235 // 7 + 1 in gv.tolist()
    finally:
        c.idx.release()


def test_batch_independence_and_the_shared_table(case):
    """nq = 3 equals three single calls; the same call twice is identical; an unscoped call on ANOTHER column in between
    changes nothing in either direction: a table not left empty would carry groups over."""
    c = case
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, (np.arange(N) * 2654435761 % 3001).astype(np.uint32))
    _set(c, 0, np.arange(N) % 2)
    truth = _truth_where(c, ODD)
    full = [c.idx.scores(qq) for qq in c.q]
    for column, zero in ((1, SINGLE), (2, GROUP), (2, SINGLE)):
        first = c.idx.search_batch_collapsed_where(c.q, 120, ODD, column, zero)
        _ask(c, ODD, column, zero, 120, truth, "batch")
        for qi in range(3):
            hits, groups, matched = c.idx.search_collapsed_where(c.q[qi], 120, ODD, column, zero)
            s, r, gv, g, m = _trim(first, qi, 120)
            assert (groups, matched) == (g, m) and [h[1] for h in hits] == r.tolist() and [h[2] for h in hits] == gv.tolist()
            assert _canon(np.array([h[0] for h in hits], dtype=np.float32)) == _canon(s)
        other = 3 - column
        us, ur, uv, ucounts, ugroups = c.idx.search_batch_collapsed(c.q, 120, other, zero)
        for qi in range(3):
            exp = collapse_model.collapsed(full[qi], c.cols[other], None, zero == SINGLE, 120)
            cnt = int(ucounts[qi])
            assert (ur[qi, :cnt].tolist(), uv[qi, :cnt].tolist(), int(ugroups[qi])) == (exp[1].tolist(), exp[2].tolist(), exp[3])
            assert _canon(us[qi, :cnt]) == _canon(exp[0])
        again = c.idx.search_batch_collapsed_where(c.q, 120, ODD, column, zero)
        for x, y in zip(first[:5], again[:5]):
            assert x.tobytes() == y.tobytes()
        assert first[5] == again[5]
    a = c.idx.search_batch_collapsed_where(c.q[::-1], 120, ODD, 2, SINGLE)
    b = c.idx.search_batch_collapsed_where(c.q, 120, ODD, 2, SINGLE)
    for x, y in zip(a[:5], b[:5]):
        assert x[::-1].tolist() == y.tolist()
    del v1, v2


def test_two_threads_one_scoped_one_unscoped(case):
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, np.arange(N) % 911)
    _set(c, 0, np.arange(N) % 2)
    truth = _truth_where(c, ODD)
    want_scoped = collapsed_scoped(truth[0][0], c.cols[1], None, truth[1], True, 150)
    want_plain = collapse_model.collapsed(c.idx.scores(c.q[1]), v2, None, False, 150)
    got, errors = [[], []], []

    def scoped():
        try:
            for _ in range(6):
                got[0].append(_trim(c.idx.search_batch_collapsed_where(c.q[:1], 150, ODD, 1, SINGLE), 0, 150))
        except BaseException as e:          # noqa: BLE001 -- reported below
            errors.append(e)

    def plain():
        try:
            for _ in range(6):
                s, r, v, counts, groups = c.idx.search_batch_collapsed(c.q[1:2], 150, 2, GROUP)
                got[1].append((s[0, :counts[0]], r[0, :counts[0]], v[0, :counts[0]], int(groups[0])))
        except BaseException as e:          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=scoped), threading.Thread(target=plain)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got[0]) == len(got[1]) == 6
    for a in got[0]:
        _same(a, want_scoped, (c.dtype, "scoped thread"))
    for s, r, v, g in got[1]:
        assert (r.tolist(), v.tolist(), g) == (want_plain[1].tolist(), want_plain[2].tolist(), want_plain[3]) and _canon(s) == _canon(want_plain[0])


def test_rows_equal_where(gpu, data, case):
    """Identity (c): the row-list entry over S shuffled and duplicated equals the predicate entry, bit for bit; with a
    row offset, after append and after compact."""
    m, q = data
    off = 1_000_000
    c = _case(m[:9000], q, case.dtype, row_offset=off)
    try:
        def both(what, n=80):
            S = np.flatnonzero(where_mask(c.cols, ODD, c.n) & ~c.dead) + off
            rng = np.random.default_rng(3)
            rows = rng.permutation(np.concatenate([S, S[::3], S[:10]]))
            for zero in (SINGLE, GROUP):
                a = c.idx.search_batch_collapsed_where(c.q, n, ODD, 1, zero)
                b = c.idx.search_batch_collapsed_within(c.q, n, rows, 1, zero)
                for qi in range(3):
                    x, y = _trim(a, qi, n), _trim(b, qi, n)
                    assert (x[3], x[4]) == (y[3], y[4]) == (y[3], len(S)), what
                    assert x[1].tolist() == y[1].tolist() and x[2].tolist() == y[2].tolist() and _canon(x[0]) == _canon(y[0]), what
                    assert (x[1] >= off).all()
                _ask(c, ODD, 1, zero, n, what=what)
                _ask_rows(c, rows, 1, zero, n, what=what)

        _set(c, 1, np.arange(9000) // 6 + 1)
        _set(c, 0, np.arange(9000) % 2)
        both("row_offset")
        c.idx.append(m[9000:9500])                                  # the new rows carry 0 in every column: out of scope
        c.n, c.dead = 9500, np.concatenate([c.dead, np.zeros(500, dtype=bool)])
        c.cols = {k: np.concatenate([v, np.zeros(500, dtype=np.uint32)]) for k, v in c.cols.items()}
        c.idx.set_column(0, np.ones(500, dtype=np.uint32), off + 9000)          # ... until their scope flag is set
        c.cols[0][9000:] = 1
        both("append", 3000)
        dead = np.zeros(9500, dtype=bool)
        dead[[1, 55, 123, 4001, 9499]] = True
        dead[2000:2600] = True
        _mask(c, np.flatnonzero(dead))
        both("masked", 200)
        c.idx.compact()
        keep = np.flatnonzero(~dead)
        c.n, c.dead = len(keep), np.zeros(len(keep), dtype=bool)
        c.cols = {k: v[keep] for k, v in c.cols.items()}
        for k, v in c.cols.items():
            assert c.idx.column(k).tolist() == v.tolist()
        both("compacted", 200)
    finally:
        c.idx.release()


def test_four_terms_and_a_large_set(gpu, data, case):
    """test_where_gpu.py's four-term predicates and its 1,024-member IN set, columns drawn from its VALUES."""
    m, q = data
    c = _case(m[:6151], q, case.dtype)                              # three filter strips + 7
    try:
        rng = np.random.default_rng(77)
        for col in (0, 1):
            _set(c, col, VALUES[rng.integers(0, len(VALUES), c.n)])
        _set(c, 2, np.arange(c.n) // 5)                             # the groups: value 0 among them
        four = [w for fam, w in PREDICATES if fam == "and" and len(w) == 4]
        big = [w for fam, w in PREDICATES if len(w) == 1 and w[0][1] == "in" and len(w[0][2]) == 1024]
        assert len(four) == 3 and len(big) == 1
        # (column 3 is never set here and reads 0, as the model says)
        for where in four[1:2] + big:
            for zero in (SINGLE, GROUP):
                got = _ask(c, where, 2, zero, 150, what="a sweep predicate")
                assert 0 < got[4] < c.n
    finally:
        c.idx.release()


def test_launch_record(case):
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    _set(c, 0, np.arange(N) % 2)
    m = N // 2
    c.idx.search_batch_collapsed_where(c.q, 5, ODD, 1, SINGLE)
    rec = _native.last_launches()
    names = [k for k, _, _ in rec]
    assert names[:2] == ["where_count_kernel", "scoped_write_kernel"] and rec[0][1:] == (N, 1) and rec[1][1:] == (N, 1)
    assert names[2].startswith("gather_scores_kernel") and rec[2][1:] == (m, 3)
    assert rec[3:] == [("collapse_reduce_kernel", m, 1), ("collapse_mark_kernel", m, 1)] * 3
    assert "gemv" not in names and not any("where_write" in k or "label_write" in k for k in names)
    c.idx.search_batch_within(c.q, 5, np.arange(1, N, 2))
    assert _native.last_launches()[0][0] == names[2]                 # the kernel svs_index_search_rows runs
    # a count-only call runs reduce and mark; there is nothing else to record
    s, r, gv, counts, groups, matched = c.idx.search_batch_collapsed_where(c.q[:1], 0, ODD, 1, SINGLE)
    names = [k for k, _, _ in _native.last_launches()]
    assert names[:2] == ["where_count_kernel", "scoped_write_kernel"] and names[2].startswith("gather_scores_kernel")
    assert names[3:] == ["collapse_reduce_kernel", "collapse_mark_kernel"]
    assert (s.shape, counts.tolist(), groups.tolist(), matched) == ((1, 0), [0], [(N + 6) // 7], m)
    # the row-list entry
    c.idx.search_batch_collapsed_within(c.q[:2], 5, np.arange(1, N, 2), 1, GROUP)
    rec = _native.last_launches()
    assert rec[0] == ("scoped_values_kernel", m, 1) and rec[1][0].startswith("gather_scores_kernel") and rec[1][1:] == (m, 2)
    assert rec[2:] == [("collapse_reduce_kernel", m, 1), ("collapse_mark_kernel", m, 1)] * 2
    # the stage times of a timed call
    c.idx.set_timing(1)
    try:
        c.idx.search_batch_collapsed_where(c.q, 5, ODD, 1, SINGLE)
        ms = (C.c_double * 6)()
        assert _native.load().svs_internal_collapse_scope_kernel_ms(ms) == 0 and all(0.0 < x < 1000.0 for x in ms), list(ms)
        c.idx.search_batch_collapsed_where(c.q, 0, ODD, 1, SINGLE)
        assert _native.load().svs_internal_collapse_scope_kernel_ms(ms) == 0 and ms[5] == -1.0 and all(x > 0.0 for x in list(ms)[:5])
    finally:
        c.idx.set_timing(0)
    c.idx.search_batch_collapsed_where(c.q, 5, ODD, 1, SINGLE)
    assert _native.load().svs_internal_collapse_scope_kernel_ms(ms) == 0 and list(ms) == [-1.0] * 6


# ---- the raw entries: every argument error leaves every output at its sentinel and launches nothing
def _term(column=0, op=0, negate=0, a=0, b=0, members=None, nset=None, keep=None):
    t = _native.WhereTerm()
    t.column, t.op, t.negate, t.a, t.b = column, op, negate, a, b
    arr = None if members is None else np.ascontiguousarray(members, dtype=np.uint32)
    if keep is not None and arr is not None:
        keep.append(arr)
    t.set = arr.ctypes.data if arr is not None and len(arr) else None
    t.nset = (len(arr) if arr is not None else 0) if nset is None else nset
    return t


class _Raw:
    """Both entries with sentinel-filled outputs."""

    def __init__(self, idx, q, k=4):
        self.idx, self.q, self.k = idx, np.ascontiguousarray(q, dtype=np.float32), k

    def _fresh(self):
        nq, k = len(self.q), self.k
        self.outs = (np.full((nq, k), -7.0, dtype=np.float32), np.full((nq, k), -7, dtype=np.int64), np.full((nq, k), 7, dtype=np.uint32))
        self.counts, self.groups, self.matched = np.full(nq, -7, dtype=np.int32), np.full(nq, -7, dtype=np.int64), C.c_int64(-7)

    def _tail(self, column, zero_mode, outs, counts):
        p = lambda a: None if a is None else a.ctypes.data
        outs = self.outs if outs is None else outs
        return (column, zero_mode, *[p(o) for o in outs], p(self.counts) if counts else None, p(self.groups), C.byref(self.matched))

    def where(self, terms, column=1, zero_mode=1, nterms=None, nq=None, d=None, k=None, q=True, outs=None, counts=True):
        self._fresh()
        arr = (_native.WhereTerm * max(len(terms), 1))(*terms) if terms is not None else None
        rc = self.idx._lib.svs_index_search_collapsed_where(
            self.idx._handle(), self.q.ctypes.data if q else None, len(self.q) if nq is None else nq, self.q.shape[1] if d is None else d,
            self.k if k is None else k, arr, (len(terms) if terms is not None else 0) if nterms is None else nterms,
            *self._tail(column, zero_mode, outs, counts))
        self.launches = _native.last_launches()
        return rc

    def rows(self, rows, column=1, zero_mode=1, nrows=None, nq=None, d=None, k=None, q=True, outs=None, counts=True):
        self._fresh()
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        rc = self.idx._lib.svs_index_search_collapsed_rows(
            self.idx._handle(), self.q.ctypes.data if q else None, len(self.q) if nq is None else nq, self.q.shape[1] if d is None else d,
            self.k if k is None else k, None if r is None else r.ctypes.data, (0 if r is None else len(r)) if nrows is None else nrows,
            *self._tail(column, zero_mode, outs, counts))
        self.launches = _native.last_launches()
        return rc

    def untouched(self):
        o = self.outs
        return bool((o[0] == -7).all() and (o[1] == -7).all() and (o[2] == 7).all() and (self.counts == -7).all()
                    and (self.groups == -7).all() and self.matched.value == -7)


def test_argument_errors_leave_the_outputs_untouched(case):
    c = case
    _set(c, 0, np.arange(N) % 2)
    INV, SHAPE, UNSUP = _native.SVS_ERR_INVALID, _native.SVS_ERR_SHAPE, _native.SVS_ERR_UNSUPPORTED
    raw = _Raw(c.idx, c.q[:2])
    keep = []
    ok = [_term(0, 0, members=[1], keep=keep)]
    some = [1, 5, 9]

    def failed(rc, want):
        assert rc == want, (rc, want, _native.last_error())
        assert raw.untouched() and raw.launches == []
        return _native.last_error()

    for call, scope in ((raw.where, ok), (raw.rows, some)):
        failed(call(scope, d=D + 1), SHAPE)
        failed(call(scope, nq=-1), INV)
        failed(call(scope, q=False), INV)
        for column in (-1, 4, 1 << 20):
            assert "column" in failed(call(scope, column=column), INV)
        for mode in (-1, 2, 77):
            assert "zero_mode" in failed(call(scope, zero_mode=mode), INV)
        failed(call(scope, counts=False), INV)
        for missing in range(3):
            raw._fresh()
            part = tuple(None if i == missing else x for i, x in enumerate(raw.outs))
            assert call(scope, outs=part) == INV and raw.launches == []
        # nq == 0: SVS_OK, nothing launched, nothing written
        assert call(scope, nq=0) == 0 and raw.untouched() and raw.launches == []
    # the predicate's errors name the new entry
    entry = "svs_index_search_collapsed_where"
    failed(raw.where(ok, nterms=-1), INV)
    failed(raw.where(None, nterms=2), INV)
    assert entry in failed(raw.where([_term(9, 0, members=[1], keep=keep)]), INV)
    assert entry in failed(raw.where([_term(0, 7)]), INV)
    assert entry in failed(raw.where([_term(0, 1, negate=2)]), INV)
    failed(raw.where([_term(0, 0, nset=-1)]), INV)
    failed(raw.where([_term(0, 0, nset=3)]), INV)                   # a null set with members
    assert entry in failed(raw.where([_term(0, 1, a=0, b=9)] * 5), UNSUP)
    assert entry in failed(raw.where([_term(0, 0, members=range(1025), keep=keep)]), UNSUP)
    # the list's errors
    failed(raw.rows(some, nrows=-1), INV)
    failed(raw.rows(None, nrows=3), INV)
    for bad in (-1, N, 1 << 40):
        failed(raw.rows([1, bad, 5]), INV)
    # an empty index; rows of more than 16 KiB
    empty = svs_amd.DeviceIndex.empty(D)
    wide = svs_amd.DeviceIndex(_unit(np.random.default_rng(2).standard_normal((8, 4100))))
    try:
        raw_e = _Raw(empty, c.q[:2])
        for rc in (raw_e.where(ok), raw_e.rows([])):
            assert rc == SHAPE and raw_e.untouched() and raw_e.launches == []
        raw_w = _Raw(wide, np.zeros((2, 4100), dtype=np.float32))
        for k in (4, 0):
            for rc in (raw_w.where(ok, k=k), raw_w.rows([1, 2], k=k)):
                assert rc == UNSUP and raw_w.untouched() and raw_w.launches == [], _native.last_error()
    finally:
        empty.release()
        wide.release()
    # successful raw calls: entries past the count stay untouched; out_groups and out_matched may be NULL
    assert raw.where(ok, column=NEVER_SET, zero_mode=0) == 0, _native.last_error()
    assert raw.counts.tolist() == [1, 1] and raw.groups.tolist() == [1, 1] and raw.matched.value == N // 2
    assert (raw.outs[1][:, 1:] == -7).all() and (raw.outs[0][:, 1:] == -7).all() and (raw.outs[2][:, 1:] == 7).all()
    assert raw.rows([], k=3) == 0 and raw.counts.tolist() == [0, 0] and raw.groups.tolist() == [0, 0] and raw.matched.value == 0
    assert raw.launches == [] and (raw.outs[1] == -7).all()
    # the Python layer's ValueErrors
    for bad in (-1, 4, True, "1"):
        with pytest.raises(ValueError):
            c.idx.search_collapsed_where(c.q[0], 3, ODD, bad)
        with pytest.raises(ValueError):
            c.idx.search_collapsed_within(c.q[0], 3, some, bad)
    with pytest.raises(ValueError):
        c.idx.search_collapsed_where(c.q[0], 3, ODD, 1, "both")
    with pytest.raises(ValueError):
        c.idx.search_collapsed_where(c.q[0], 3, [(0, "between", (1, 2))], 1)
    with pytest.raises(ValueError):
        c.idx.search_collapsed_where(c.q, 3, ODD, 1)                  # a 2-D query
    with pytest.raises(ValueError):
        c.idx.search_collapsed_within(c.q, 3, some, 1)
    hits, groups, matched = c.idx.search_collapsed_within(c.q[0], 3, [N - 1, 4, N - 1], NEVER_SET, GROUP)
    assert (groups, matched) == (1, 2) and [(r, v) for _, r, v in hits] == [(N - 1, 0)] and isinstance(hits[0][0], float)

"""GPU: the collapsed search (svs_index_search_collapsed; svs_amd/csrc/collapse.h) against its definition.

The truth is ``idx.scores(q)`` (svs_index_scores_n: the same kernel), ``idx.column(c)`` and the masked rows fed to the
numpy model (collapse_model.py): rows, values, counts and groups must be EQUAL, score bits equal with NaN
canonicalised as in test_by_label_gpu.py.  No tolerances.

Shape: N = 24,579 rows (24 strips of 1,024 rows + 3: no multiple of 4, several strips, the last strip holds 3 rows) of
64 unit-norm Gaussian elements, under f32, f16 and fp8, 3 queries.  Row N - 1 (in the tail) IS query 0, so it is the
best row of the corpus; rows 17 and 20000 are one vector, rows 33 and 15000 another, both close to query 0.  The kernels
stride over strips (CL_GRID_MAX workgroups at most), so one more case, ``test_several_strips_per_workgroup``, has
n = 2 * CL_GRID_MAX * CL_STRIP + CL_STRIP + 3 rows, read from the library.

Columns 1 and 2 are written by the tests as they need them; column 3 is NEVER set by any test of this file."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest

import collapse_model
import select_cases
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N, D = 24579, 64
DTYPES = ["f32", "f16", "fp8"]
TOP = 0xFFFFFFFF
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


@pytest.fixture(scope="module", params=DTYPES)
def case(request, gpu, data):
    m, q = data
    idx = svs_amd.DeviceIndex(m, dtype=request.param)
    s = [idx.scores(qq) for qq in q]          # the reference, computed once, never written
    for v in s:
        v.setflags(write=False)
    yield SimpleNamespace(idx=idx, s=s, m=m, q=q, dtype=request.param)
    idx.release()


def _canon(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32)).tolist()


def _check(got, exp, what, row_offset=0):
    s, r, v, g = got
    es, er, ev, eg = exp
    assert g == eg, (what, g, eg)
    assert r.tolist() == (er + row_offset).tolist(), what
    assert v.tolist() == ev.tolist(), what
    assert _canon(s) == _canon(es), what


def _one(idx, q, n, column, zero):
    """One query through the Python entry: (scores, rows, values, groups), trimmed to the count."""
    s, r, v, counts, groups = idx.search_batch_collapsed(q[None, :], n, column, zero)
    c = int(counts[0])
    assert c == min(max(n, 0), int(groups[0]), s.shape[1])
    return s[0, :c], r[0, :c], v[0, :c], int(groups[0])


def _ask(c, qi, column, values, zero, n, dead=None, what=None):
    """One query, checked against the model over ``values`` (what the test wrote into ``column``; None: never set)."""
    got = _one(c.idx, c.q[qi], n, column, zero)
    exp = collapse_model.collapsed(c.s[qi], values, dead, zero == SINGLE, n)
    _check(got, exp, (c.dtype, what, zero, n))
    return got


def _set(c, column, values):
    values = np.ascontiguousarray(values, dtype=np.uint32)
    c.idx.set_column(column, values)
    assert c.idx.column(column).tolist() == values.tolist()
    return values


def _raw(idx, q, k, column, zero_mode, outs, counts, groups, d=None, nq=None):
    q = np.ascontiguousarray(q, dtype=np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    return idx._lib.svs_index_search_collapsed(idx._handle(), q.ctypes.data, q.shape[0] if nq is None else nq, q.shape[1] if d is None else d,
                                               k, column, zero_mode, *[p(o) for o in outs], p(counts), p(groups))


def _fresh(nq, k):
    outs = (np.full((nq, k), -7.0, dtype=np.float32), np.full((nq, k), -7, dtype=np.int64), np.full((nq, k), 7, dtype=np.uint32))
    return outs, np.full(nq, -7, dtype=np.int32), np.full(nq, -7, dtype=np.int64)


def _untouched(outs, counts=None, groups=None, frm=0):
    ok = (outs[0][..., frm:] == -7).all() and (outs[1][..., frm:] == -7).all() and (outs[2][..., frm:] == 7).all()
    return ok and (counts is None or (counts == -7).all()) and (groups is None or (groups == -7).all())


def test_adjacent_runs(case):
    """Runs of 7 rows: 4 does not divide 7 and 64 * 4 is no multiple of it, so runs straddle a thread's four rows, a
    wave, a strip and a workgroup.  Catches errors in the thread's fold and in the wave merge."""
    c = case
    v = _set(c, 1, np.arange(N) // 7 + 1)
    groups = (N + 6) // 7
    for qi in range(3):
        for zero in (SINGLE, GROUP):
            got = _ask(c, qi, 1, v, zero, 100, what="runs of 7")
            assert got[3] == groups and len(set(got[2].tolist())) == 100
    assert _ask(c, 0, 1, v, SINGLE, 100)[1][0] == N - 1
    # runs of 64 and of 256 rows: whole waves and whole workgroups on one value; runs of 3: several values in a thread
    for run in (64, 256, 3):
        v = _set(c, 1, np.arange(N) // run + 1)
        assert _ask(c, 1, 1, v, SINGLE, 150, what=("runs", run))[3] == (N + run - 1) // run


def test_groups_in_far_apart_strips(case):
    """One vector twice under ONE value in strips 0 and 19: the tie goes to the larger row.  One vector under TWO
    values: both appear, the larger row first.  Catches a maximum taken on the score instead of the key."""
    c = case
    s = c.s[0]
    assert s[17].view(np.uint32) == s[20000].view(np.uint32) and s[33].view(np.uint32) == s[15000].view(np.uint32)
    vals = np.arange(N, dtype=np.uint32) + 1
    vals[20000] = vals[17]
    v = _set(c, 1, vals)
    sc, r, gv, g = _ask(c, 0, 1, v, SINGLE, 50, what="far apart")
    rows = r.tolist()
    assert g == N - 1 and 20000 in rows and 17 not in rows and gv[rows.index(20000)] == 18
    i = rows.index(15000)
    assert rows[i + 1] == 33 and sc[i].view(np.uint32) == sc[i + 1].view(np.uint32) and gv[i] != gv[i + 1]


def test_one_giant_group(case):
    """Every second row carries one value, every other row its own: contention on one slot of the table."""
    c = case
    vals = np.arange(N, dtype=np.uint32) + 1
    vals[::2] = 4_000_000
    v = _set(c, 1, vals)
    for qi in range(3):
        got = _ask(c, qi, 1, v, SINGLE, 200, what="giant")
        assert got[3] == N // 2 + 1 and got[2].tolist().count(4_000_000) == 1
    # the giant group alone (every row): one hit, the best row
    v = _set(c, 1, np.full(N, 4_000_000))
    sc, r, gv, g = _ask(c, 0, 1, v, SINGLE, 10, what="one value")
    assert (r.tolist(), gv.tolist(), g) == ([N - 1], [4_000_000], 1)


def test_every_row_its_own_value(case):
    """The table at its fullest.  The answer is the plain top-k, and groups is the live row count."""
    c = case
    v = _set(c, 1, np.arange(N) + 1)
    for qi in range(3):
        sc, r, gv, g = _ask(c, qi, 1, v, SINGLE, 100, what="unique")
        ps, pr = c.idx.search_batch(c.q[qi:qi + 1], 100)
        assert g == N and r.tolist() == pr[0].tolist() and _canon(sc) == _canon(ps[0]) and gv.tolist() == (r + 1).tolist()
    assert _ask(c, 2, 1, v, GROUP, 100, what="unique, 0 is a group")[3] == N


def test_values_that_collide_under_any_power_of_two_reduction(case):
    """1,024 rows carry i << 22 (their low 22 bits are equal), the others 0xFFFFFFFF or 1: a table indexed by the low
    bits of the value puts them all into one chain."""
    c = case
    vals = np.where(np.arange(N) % 3 == 0, TOP, 1).astype(np.uint32)
    at = np.arange(1024) * 24
    vals[at] = (np.arange(1024, dtype=np.uint32) << np.uint32(22))
    v = _set(c, 1, vals)
    for zero, groups in ((SINGLE, 1023 + 1 + 2), (GROUP, 1024 + 2)):      # (0 << 22 is the value 0: one row)
        for qi in (0, 1):
            sc, r, gv, g = _ask(c, qi, 1, v, zero, 2000, what="colliding values")
            assert g == groups == len(r) and {TOP, 1, 0, 5 << 22} <= set(gv.tolist())
    v = _set(c, 1, np.where(np.arange(N) % 2 == 0, TOP, TOP - 1))
    assert _ask(c, 1, 1, v, SINGLE, 5, what="two top values")[3] == 2


def test_value_zero(case):
    """Value 0 on rows 50 .. 59 and on the best row: one hit under ZERO_IS_GROUP, each of them under ZERO_SINGLE."""
    c = case
    vals = (np.arange(N) // 7 + 1).astype(np.uint32)
    vals[50:60] = 0
    vals[N - 1] = 0
    v = _set(c, 1, vals)
    others = len(set(vals.tolist())) - 1
    sc, r, gv, g = _ask(c, 0, 1, v, GROUP, N, what="0 is a group")
    assert g == others + 1 and gv.tolist().count(0) == 1 and r[0] == N - 1 and gv[0] == 0
    sc, r, gv, g = _ask(c, 0, 1, v, SINGLE, N, what="0 stands alone")
    assert g == others + 11 and sorted(r[gv == 0].tolist()) == list(range(50, 60)) + [N - 1] and r[0] == N - 1
    for qi in (1, 2):
        for zero in (SINGLE, GROUP):
            _ask(c, qi, 1, v, zero, 300, what="zeros")


def test_column_never_set(case):
    """ZERO_SINGLE: the plain top-k, rows and score bits.  ZERO_IS_GROUP: one hit, the best live row."""
    c = case
    assert not c.idx.column(NEVER_SET).any()
    for qi in range(3):
        for k in (1, 100, 2049):
            sc, r, gv, g = _ask(c, qi, NEVER_SET, None, SINGLE, k, what="never set")
            ps, pr = c.idx.search_batch(c.q[qi:qi + 1], k)
            assert g == N and r.tolist() == pr[0].tolist() and _canon(sc) == _canon(ps[0]) and not gv.any()
        sc, r, gv, g = _ask(c, qi, NEVER_SET, None, GROUP, 100, what="never set, one group")
        ps, pr = c.idx.search_batch(c.q[qi:qi + 1], 1)
        assert (r.tolist(), gv.tolist(), g) == (pr[0].tolist(), [0], 1) and _canon(sc) == _canon(ps[0])


def test_tombstones(gpu, data, case):
    """A masked best row hands over to the runner-up (its own score bits); a group masked whole is absent and groups
    drops by one; a dead row never comes back through its score."""
    m, q = data
    dtype = case.dtype
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        c = SimpleNamespace(idx=idx, s=case.s, q=q, dtype=dtype)
        vals = (np.arange(N) // 7 + 1).astype(np.uint32)
        vals[50:60] = 0
        v = _set(c, 2, vals)
        dead = np.zeros(N, dtype=bool)
        before = _ask(c, 0, 2, v, SINGLE, 40, what="before")
        top_value = int(vals[N - 1])
        assert before[1][0] == N - 1 and before[2][0] == top_value
        dead[N - 1] = True
        idx.mask_rows([N - 1])
        after = _ask(c, 0, 2, v, SINGLE, N, dead=dead, what="best row masked")
        i = after[2].tolist().index(top_value)
        assert after[3] == before[3] and after[1][i] == N - 2      # (the run holds rows N - 2 and N - 1)
        assert after[0][i].view(np.uint32) == case.s[0][N - 2].view(np.uint32)              # the runner-up's own bits
        dead[np.nonzero(vals == top_value)[0]] = True            # the rest of that group
        idx.mask_rows(np.nonzero(vals == top_value)[0])
        gone = _ask(c, 0, 2, v, SINGLE, N, dead=dead, what="group masked")
        assert gone[3] == before[3] - 1 and top_value not in gone[2].tolist()
        # exempt rows die alone; each of the four nibble positions, a whole bitmap word; then a random 5 %
        more = [52, 57, 1000, 1001, 1002, 1003, 2005, 2010, 2015, 2016] + list(range(6400, 6432))
        dead[more] = True
        idx.mask_rows(more)
        for zero in (SINGLE, GROUP):
            _ask(c, 0, 2, v, zero, 500, dead=dead, what="nibbles")
        rnd = np.nonzero((np.random.default_rng(8).random(N) < 0.05) & ~dead)[0]
        dead[rnd] = True
        idx.mask_rows(rnd)
        for qi in range(3):
            got = _ask(c, qi, 2, v, SINGLE, N, dead=dead, what="5 % masked")
            assert not dead[got[1]].any() and len(got[1]) == got[3]
        # never set + tombstones: the masked plain top-k
        sc, r, gv, g = _ask(c, 1, NEVER_SET, None, SINGLE, 100, dead=dead, what="never set, masked")
        ps, pr = idx.search_batch(q[1:2], 100)
        assert g == int((~dead).sum()) and r.tolist() == pr[0].tolist() and _canon(sc) == _canon(ps[0])
    finally:
        idx.release()


def test_counts_and_every_route_of_the_selection_stage(gpu, data, case):
    c = case
    # k larger than |W| on a 5-group column: count 5, the entries past it hold the caller's sentinel
    v = _set(c, 1, np.arange(N) % 5 + 10)
    exp = collapse_model.collapsed(c.s[2], v, None, True, 100)
    for k in (9, 5, 3, 1):
        outs, counts, groups = _fresh(1, k)
        assert _raw(c.idx, c.q[2:3], k, 1, 1, outs, counts, groups) == 0, _native.last_error()
        cnt = min(k, 5)
        assert counts.tolist() == [cnt] and groups.tolist() == [5]
        _check(tuple(o[0, :cnt] for o in outs) + (5,), tuple(e[:cnt] for e in exp[:3]) + (5,), (c.dtype, "k", k))
        assert _untouched(outs, frm=cnt)
    # k = 0 and k < 0: count-only, null result pointers; out_groups may be NULL
    for k in (0, -4):
        counts, groups = np.full(1, -7, dtype=np.int32), np.full(1, -7, dtype=np.int64)
        assert _raw(c.idx, c.q[2:3], k, 1, 1, (None,) * 3, counts, groups) == 0, _native.last_error()
        assert counts.tolist() == [0] and groups.tolist() == [5]
    counts = np.full(1, -7, dtype=np.int32)
    assert _raw(c.idx, c.q[2:3], 0, 1, 1, (None,) * 3, counts, None) == 0 and counts.tolist() == [0]
    assert _one(c.idx, c.q[2], 0, 1, SINGLE)[3] == 5
    # nq == 0: nothing launched, nothing written
    outs, counts, groups = _fresh(2, 3)
    assert _raw(c.idx, c.q[:2], 3, 1, 1, outs, counts, groups, nq=0) == 0
    assert _untouched(outs, counts, groups) and _native.last_launches() == []
    # the window route (n > SORT_CAP, k <= SEL_KMAX), k on both sides of the emit boundary; the sorted route (k > SEL_KMAX)
    ks = sorted({cs.k for cs in select_cases.SCORE_CASES if cs.name in ("gauss-k1", "gauss-k100", "gauss-k257", "gauss-k2048", "gauss-k2049")})
    assert ks == [1, 100, 257, 2048, 2049]
    v = _set(c, 1, np.arange(N) // 3 + 1)                        # 8,193 groups: every k is cut by k, not by |W|
    for k in ks:
        for qi in (0, 1):
            assert len(_ask(c, qi, 1, v, SINGLE, k, what=("route", k))[1]) == k
    # ... and with fewer groups than k: the struck rows fill the selection, the host trims
    v5 = _set(c, 1, np.arange(N) % 5 + 10)
    for k in (100, 2049):
        assert len(_ask(c, 0, 1, v5, GROUP, k, what=("few groups", k))[1]) == 5
    # one workgroup reads the scores (n <= SORT_CAP): select_cases' path D size 4095
    n_d = max(n for n in select_cases.D_SIZES if n % 4)
    small = svs_amd.DeviceIndex(data[0][:n_d], dtype=c.dtype)
    try:
        cs = SimpleNamespace(idx=small, s=[small.scores(qq) for qq in c.q], q=c.q, dtype=c.dtype)
        vs = _set(cs, 1, np.arange(n_d) // 5 + 1)
        for k in (1, 100, n_d):
            assert len(_ask(cs, 1, 1, vs, SINGLE, k, what=("path D", k))[1]) == min(k, (n_d + 4) // 5)
        _ask(cs, 2, NEVER_SET, None, SINGLE, n_d, what="path D, never set")
    finally:
        small.release()


def test_batch_independence(case):
    """nq = 3 equals three single calls; the same call twice gives the same answer and so does a call on ANOTHER column
    in between: a table not left empty would carry groups over."""
    c = case
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, (np.arange(N) * 2654435761 % 3001).astype(np.uint32))      # 3,001 scattered groups, 0 among them
    for column, v in ((1, v1), (2, v2), (1, v1), (NEVER_SET, None), (2, v2)):
        for zero in (SINGLE, GROUP):
            for _ in range(2):
                s, r, gv, counts, groups = c.idx.search_batch_collapsed(c.q, 120, column, zero)
                for qi in range(3):
                    exp = collapse_model.collapsed(c.s[qi], v, None, zero == SINGLE, 120)
                    cnt = int(counts[qi])
                    _check((s[qi, :cnt], r[qi, :cnt], gv[qi, :cnt], int(groups[qi])), exp, (c.dtype, "batch", column, zero, qi))
                    _check(_one(c.idx, c.q[qi], 120, column, zero), exp, (c.dtype, "alone", column, zero, qi))
    a = c.idx.search_batch_collapsed(c.q[::-1], 120, 2, SINGLE)
    b = c.idx.search_batch_collapsed(c.q, 120, 2, SINGLE)
    for x, y in zip(a, b):
        assert x[::-1].tolist() == y.tolist()


def test_nan_score_is_the_largest(gpu, data):
    m, q = data
    mm = m[:9001].copy()
    mm[1234, 5] = np.nan
    idx = svs_amd.DeviceIndex(mm, dtype="f32")
    try:
        s = idx.scores(q[2])
        assert np.isnan(s[1234])
        c = SimpleNamespace(idx=idx, s=[None, None, s], q=q, dtype="f32")
        v = _set(c, 1, np.arange(9001) // 7 + 1)
        sc, r, gv, g = _ask(c, 2, 1, v, SINGLE, 10, what="nan")
        assert r[0] == 1234 and np.isnan(sc[0]) and gv[0] == 1234 // 7 + 1 and not set(range(1232, 1239)) & set(r[1:].tolist())
    finally:
        idx.release()


def test_row_offset_append_and_compact(gpu, data, case):
    m, q = data
    dtype = case.dtype
    off = 1_000_000
    idx = svs_amd.DeviceIndex(m[:9000], dtype=dtype, row_offset=off)
    try:
        vals = (np.arange(9000) // 6 + 1).astype(np.uint32)
        idx.set_column(1, vals)
        s = idx.scores(q[1])
        got = _one(idx, q[1], 80, 1, SINGLE)
        _check(got, collapse_model.collapsed(s, vals, None, True, 80), "row_offset", row_offset=off)
        assert (got[1] >= off).all()
        # after append: the new rows carry 0 -- each its own group, or one group; the table grows with the rows
        idx.append(m[9000:9500])
        s2 = idx.scores(q[1])
        vals2 = np.concatenate([vals, np.zeros(500, dtype=np.uint32)])
        for zero, groups in ((SINGLE, 1500 + 500), (GROUP, 1500 + 1)):
            got = _one(idx, q[1], 3000, 1, zero)
            _check(got, collapse_model.collapsed(s2, vals2, None, zero == SINGLE, 3000), ("append", zero), row_offset=off)
            assert got[3] == groups
        # after compact: the values move with the rows
        dead = np.zeros(9500, dtype=bool)
        dead[[0, 55, 123, 4000, 9499]] = True
        dead[2000:2600] = True
        idx.mask_rows(np.nonzero(dead)[0] + off)
        _check(_one(idx, q[1], 200, 1, SINGLE), collapse_model.collapsed(s2, vals2, dead, True, 200), "masked", row_offset=off)
        idx.compact()
        keep = np.nonzero(~dead)[0]
        s3 = idx.scores(q[1])
        _check(_one(idx, q[1], 200, 1, SINGLE), collapse_model.collapsed(s3, vals2[keep], None, True, 200), "compacted", row_offset=off)
    finally:
        idx.release()


def test_two_threads_on_one_handle_with_different_columns(case):
    """Each context owns its table: concurrent calls on different columns must not see each other's groups."""
    c = case
    v1 = _set(c, 1, np.arange(N) // 7 + 1)
    v2 = _set(c, 2, np.arange(N) % 911)
    asks = [(0, 1, v1, SINGLE), (1, 2, v2, GROUP), (2, 2, v2, SINGLE), (1, NEVER_SET, None, SINGLE)]
    want = [collapse_model.collapsed(c.s[qi], v, None, zero == SINGLE, 150) for qi, _, v, zero in asks]
    got = [[] for _ in asks]
    errors = []

    def work(i):
        qi, column, _, zero = asks[i]
        try:
            for _ in range(6):
                got[i].append(_one(c.idx, c.q[qi], 150, column, zero))
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
    """The kernels under test ran: per query "gemv", its score kernel, the reduce and the mark kernel."""
    c = case
    _set(c, 1, np.arange(N) // 7 + 1)
    c.idx.search_batch_collapsed(c.q, 5, 1, SINGLE)
    rec = _native.last_launches()
    names = [k for k, _, _ in rec]
    assert [e for e in rec if e[0] == "collapse_reduce_kernel"] == [("collapse_reduce_kernel", N, 1)] * 3
    assert [e for e in rec if e[0] == "collapse_mark_kernel"] == [("collapse_mark_kernel", N, 1)] * 3
    assert names.count("gemv") == 3 and len(names) == 12, names
    kernels = [k for k in names if k not in ("gemv", "collapse_reduce_kernel", "collapse_mark_kernel")]
    assert len(kernels) == 3 and len(set(kernels)) == 1, names
    c.idx.scores(c.q[0])
    assert _native.last_launches()[1][0] == kernels[0]               # the kernel svs_index_scores_n runs
    for i in range(0, 12, 4):
        assert names[i] == "gemv" and names[i + 2:i + 4] == ["collapse_reduce_kernel", "collapse_mark_kernel"]
    # a count-only call runs them too
    c.idx.search_batch_collapsed(c.q[:1], 0, 1, SINGLE)
    assert [k for k, _, _ in _native.last_launches()][2:] == ["collapse_reduce_kernel", "collapse_mark_kernel"]


def test_argument_errors_leave_the_outputs_untouched(case):
    c = case
    k = 4
    q2 = c.q[:2]
    INV, SHAPE = _native.SVS_ERR_INVALID, _native.SVS_ERR_SHAPE

    def call(expect, *args, outs=True, counts=True, **kw):
        o, cn, g = _fresh(2, k)
        rc = _raw(c.idx, *args, o if outs is True else outs, cn if counts else None, g, **kw)
        assert rc == expect, (rc, _native.last_error())
        assert _untouched(o, cn, g) and _native.last_launches() == []
        return _native.last_error()

    call(SHAPE, np.zeros((2, D + 1), dtype=np.float32), k, 1, 1)
    call(INV, q2, k, 1, 1, nq=-1)
    for column in (-1, 4, 1 << 20):
        assert "column" in call(INV, q2, k, column, 1)
    for mode in (-1, 2, 77):
        assert "zero_mode" in call(INV, q2, k, 1, mode)
    call(INV, q2, k, 1, 1, counts=False)
    for missing in range(3):
        o, cn, g = _fresh(2, k)
        part = tuple(None if i == missing else x for i, x in enumerate(o))
        assert _raw(c.idx, q2, k, 1, 1, part, cn, g) == INV and _untouched(o, cn, g)
    o, cn, g = _fresh(2, k)
    assert c.idx._lib.svs_index_search_collapsed(c.idx._handle(), None, 2, D, k, 1, 1, *[x.ctypes.data for x in o], cn.ctypes.data,
                                                 g.ctypes.data) == INV
    assert _untouched(o, cn, g)
    empty = svs_amd.DeviceIndex.empty(D)
    try:
        o, cn, g = _fresh(2, k)
        assert _raw(empty, q2, k, 1, 1, o, cn, g) == SHAPE and _untouched(o, cn, g)
    finally:
        empty.release()
    for bad in (-1, 4, True, "1"):
        with pytest.raises(ValueError):
            c.idx.search_collapsed(c.q[0], 3, bad)
    with pytest.raises(ValueError):
        c.idx.search_collapsed(c.q[0], 3, 1, "both")
    with pytest.raises(ValueError):
        c.idx.search_collapsed(c.q, 3, 1)
    hits, groups = c.idx.search_collapsed(c.q[0], 3, NEVER_SET, GROUP)
    assert groups == 1 and [(r, v) for _, r, v in hits] == [(N - 1, 0)] and isinstance(hits[0][0], float)


def test_several_strips_per_workgroup(gpu):
    """Every workgroup of the capped grid takes two strips, the first a third, and a ragged rest of 3 rows: the strided
    loops of both kernels.  Groups of 5 (the first few of 6) scattered over the whole corpus by r % (n // 5)."""
    geo = np.zeros(2, dtype=np.int32)
    assert _native.load().svs_internal_collapse_geometry(geo.ctypes.data_as(_native.C.POINTER(_native.C.c_int32))) == 0
    strip, grid = int(geo[0]), int(geo[1])
    n = 2 * grid * strip + strip + 3
    d = 64
    rng = np.random.default_rng(78)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    q = _unit(rng.standard_normal((1, d)))
    vals = (np.arange(n) % (n // 5)).astype(np.uint32)
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    try:
        idx.set_column(1, vals)
        dead = np.zeros(n, dtype=bool)
        dead[rng.integers(0, n, 5000)] = True
        dead[[n - 1, grid * strip, grid * strip + 1]] = True
        idx.mask_rows(np.nonzero(dead)[0])
        s = idx.scores(q[0])
        for zero in (GROUP, SINGLE):
            got = _one(idx, q[0], 100, 1, zero)
            rec = _native.last_launches()
            assert rec[2] == ("collapse_reduce_kernel", n, 1) and rec[3] == ("collapse_mark_kernel", n, 1)
            _check(got, collapse_model.collapsed(s, vals, dead, zero == SINGLE, 100), ("strided", zero))
        assert got[3] >= n // 5 - 1
    finally:
        idx.release()

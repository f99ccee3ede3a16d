"""GPU: predicate search (svs_index_search_where, where.h) -- top-k over the live rows on which a conjunction of column
predicates holds, with the filter run on the device.

The core assertion is the entry's definition: the result equals ``search_batch_within`` over
``flatnonzero(model_mask & live) + row_offset`` bit for bit (scores, rows, count), ``matched`` equals the numpy count
(tests/where_model.py), and ``svs_internal_last_launches`` names both filter kernels and the gather kernel the
``search_rows`` call took.  One case is also held against ``oracle.cpu_search`` over the matching rows.  Corpus sizes
sit around the filter's workgroup strip (``svs_internal_labels_strip``)."""
import ctypes as C

import numpy as np
import pytest

from compare import assert_topk_parity
from oracle import svs_oracle as oracle
from where_model import where_mask

pytestmark = pytest.mark.gpu

D = 64
HI, TOP = 0x80000000, 0xFFFFFFFF
VALUES = np.array([0, 1, 2, 7, HI, TOP], dtype=np.uint32)
BIG = [2] + list(range(1000, 1000 + 1023))          # 1,024 members, of which the corpora carry one
TOL_F32 = 2e-6                                       # tests/test_labels_gpu.py::test_oracle_anchor's tolerance
UNSET = 2                                            # the column no test of the sweep ever sets

# (family, where).  Columns 0, 1 and 3 are drawn from VALUES, column UNSET reads 0 everywhere.
PREDICATES = [
    ("in", [(0, "in", [1])]),
    ("in", [(0, "not in", [7, 1, 7])]),
    ("in", [(3, "in", [TOP, 0, HI])]),
    ("in", [(0, "in", BIG)]),
    ("in", [(1, "in", [5])]),                                    # nothing
    ("in", [(0, "in", [])]),                                     # nothing: the empty set
    ("in", [(UNSET, "not in", [0])]),                            # nothing: the never-set column is 0
    ("in", [(1, "not in", [5, 6])]),                             # everything
    ("in", [(0, "in", VALUES.tolist())]),                        # everything
    ("in", [(UNSET, "in", [9, 0])]),                             # everything
    ("in", [(0, "not in", [])]),                                 # everything
    ("range", [(0, "range", (1, 7))]),
    ("range", [(0, "not range", (2, HI))]),
    ("range", [(3, "range", (HI, TOP))]),
    ("range", [(1, "range", (7, 1))]),                           # nothing: a > b
    ("range", [(UNSET, "range", (1, TOP))]),                     # nothing
    ("range", [(1, "range", (0, TOP))]),                         # everything
    ("range", [(1, "not range", (TOP, 0))]),                     # everything
    ("any_bits", [(0, "any_bits", 1)]),
    ("any_bits", [(0, "no_bits", HI)]),
    ("any_bits", [(3, "any_bits", 6)]),
    ("any_bits", [(1, "any_bits", 0)]),                          # nothing: mask 0
    ("any_bits", [(UNSET, "any_bits", TOP)]),                    # nothing
    ("any_bits", [(1, "no_bits", 0)]),                           # everything
    ("all_bits", [(0, "all_bits", 3)]),
    ("all_bits", [(0, "not all_bits", HI | 1)]),
    ("all_bits", [(1, "not all_bits", 0)]),                      # nothing
    ("all_bits", [(UNSET, "all_bits", 1)]),                      # nothing
    ("all_bits", [(1, "all_bits", 0)]),                          # everything
    ("all_bits", [(UNSET, "not all_bits", 4)]),                  # everything
    # two and four terms; two terms on one column; a term on the never-set column
    ("and", [(0, "in", [1, 2, 7]), (1, "range", (0, 7))]),
    ("and", [(0, "range", (1, HI)), (0, "any_bits", 1)]),
    ("and", [(1, "not in", [0]), (UNSET, "in", [0])]),
    ("and", [(0, "in", [1]), (0, "in", [2])]),                   # nothing: one value cannot be both
    ("and", [(0, "not in", [0]), (1, "no_bits", HI), (3, "range", (0, HI)), (UNSET, "in", [0, 9])]),
    ("and", [(0, "in", [0, 1, 2, 7]), (1, "not in", [TOP, 1]), (3, "not all_bits", 3), (1, "not range", (2, 2))]),
    ("and", [(3, "all_bits", 0), (1, "range", (0, TOP)), (0, "no_bits", 0), (UNSET, "not in", [])]),   # everything
]


def _strip():
    from svs_amd import _native
    r = int(_native.load().svs_internal_labels_strip())
    assert r >= 64 and r % 32 == 0
    return r


def _unit_rows(rng, n, d=D):
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


_QUERIES = _unit_rows(np.random.default_rng(5), 3)
_CORPORA = {}


def _corpus(n):
    """(rows, {column: values drawn from VALUES} for columns 0, 1 and 3) of an n-row corpus, made once."""
    if n not in _CORPORA:
        rng = np.random.default_rng(2000 + n)
        _CORPORA[n] = (_unit_rows(rng, n), {c: VALUES[rng.integers(0, len(VALUES), n)] for c in (0, 1, 3)})
    return _CORPORA[n]


def _index(m, cols, **kw):
    from svs_amd import DeviceIndex
    idx = DeviceIndex(m, **kw)
    for c, v in cols.items():
        idx.set_column(c, v)
    return idx


def _names(launches):
    return [rec[0] for rec in launches]


def _check(idx, cols, dead, q, k, where, tag):
    """One predicate call against search_batch_within over the rows the numpy model selects; returns matched."""
    from svs_amd import _native
    n = idx.n
    sel = where_mask(cols, where, n)
    if dead is not None:
        sel &= ~dead
    rows = np.flatnonzero(sel) + idx.row_offset
    s, r, matched = idx.search_batch_where(q, k, where)
    ours = _native.last_launches()
    es, er = idx.search_batch_within(q, k, rows)
    theirs = _native.last_launches()
    count = min(max(k, 0), len(rows))
    assert matched == len(rows), (tag, matched, len(rows))
    assert s.shape == es.shape == (len(q), count) and r.shape == er.shape, (tag, s.shape, es.shape)
    assert s.tobytes() == es.tobytes(), f"{tag}: score bits differ"
    assert np.array_equal(r, er), f"{tag}: rows differ"
    if count:
        assert "where_count_kernel" in _names(ours) and "where_write_kernel" in _names(ours), (tag, ours)
        gather = [rec for rec in ours if rec[0].startswith("gather_scores_kernel")]
        assert gather and gather == [rec for rec in theirs if rec[0].startswith("gather_scores_kernel")], (tag, ours, theirs)
    else:
        assert _names(ours) == ["where_count_kernel"], (tag, ours)
    return matched


def _sweep(idx, cols, dead, tag, predicates=PREDICATES, nqs=(1, 3)):
    """Every predicate with nq in nqs and k in {1, 10, m, m + 5}.  Per op family the sweep must hold a predicate nothing
    matches and one every live row matches -- and, where there are two live rows or more, one that some match and
    some do not: a sweep in which everything or nothing matches shows nothing.  (One row cannot be split.)"""
    live = idx.n - (int(dead.sum()) if dead is not None else 0)
    seen = {}
    for family, where in predicates:
        m = int((where_mask(cols, where, idx.n) & (~dead if dead is not None else True)).sum())
        seen.setdefault(family, set()).add("none" if m == 0 else "all" if m == live else "some")
        for nq in nqs:
            for k in sorted({1, 10, max(m, 1), m + 5}):
                assert _check(idx, cols, dead, _QUERIES[:nq], k, where, f"{tag} where={where if len(str(where)) < 200 else family} nq={nq} k={k}") == m
    for family in ("in", "range", "any_bits", "all_bits"):
        if family in seen:
            assert {"none", "all"} <= seen[family], (tag, family, seen[family])
            assert live < 2 or "some" in seen[family], (tag, family, seen[family])
    return seen


def _sizes():
    r = _strip()
    return [1, 63, 65, r - 1, r + 1, 3 * r + 37]


@pytest.mark.parametrize("dtype,size", [("f32", s) for s in range(6)] + [("f16", 5), ("fp8", 5)])
def test_equals_search_within_over_the_matching_rows(gpu, dtype, size):
    n = _sizes()[size]
    m, cols = _corpus(n)
    idx = _index(m, cols, dtype=dtype)
    seen = _sweep(idx, cols, None, f"{dtype} n={n}")
    assert set(seen) == {"in", "range", "any_bits", "all_bits", "and"}
    assert not idx.column(UNSET).any()
    idx.release()


def test_result_does_not_depend_on_term_order_or_set_order(gpu):
    n = 3 * _strip() + 37
    m, cols = _corpus(n)
    idx = _index(m, cols)
    where = [(0, "in", [7, 1, 2]), (1, "not in", [TOP, 1]), (3, "not all_bits", 3), (1, "not range", (2, 2))]
    want = idx.search_batch_where(_QUERIES, 25, where)
    for other in (where[::-1], [where[2], where[0], where[3], where[1]],
                  [(0, "in", [2, 2, 1, 7, 1]), (1, "not in", [1, TOP, TOP])] + where[2:]):
        got = idx.search_batch_where(_QUERIES, 25, other)
        assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2] == want[2]
    one = idx.search_batch_where(_QUERIES[1:2], 25, where)        # nor on nq
    assert one[0].tobytes() == want[0][1:2].tobytes() and np.array_equal(one[1], want[1][1:2])
    idx.release()


def test_one_in_term_on_column_0_is_the_labelled_search(gpu):
    from svs_amd import _native
    n = 3 * _strip() + 37
    m, cols = _corpus(n)
    idx = _index(m, cols)
    assert np.array_equal(idx.labels(), cols[0])                 # column 0 is the label column
    dead = np.zeros(n, dtype=bool)
    for masked in (False, True):
        if masked:
            dead[::5] = True
            idx.mask_rows(np.flatnonzero(dead))
        for label_set in ([1], [0], [2, 7], [TOP, 1, 1], BIG, [5]):
            for nq, k in ((1, 1), (3, 10), (2, n)):
                s, r, matched = idx.search_batch_where(_QUERIES[:nq], k, [(0, "in", label_set)])
                ls, lr, lmatched = idx.search_batch_labeled(_QUERIES[:nq], k, label_set)
                assert matched == lmatched == int((np.isin(cols[0], label_set) & ~dead).sum())
                assert s.tobytes() == ls.tobytes() and np.array_equal(r, lr), (label_set, nq, k)
    idx.release()


def test_row_offset(gpu):
    n = _strip() + 1
    m, cols = _corpus(n)
    idx = _index(m, cols, row_offset=1000)                       # (row0=None: from the index's first row, 1000)
    assert np.array_equal(idx.column(3, 1000 + 5, 7), cols[3][5:12])
    where = [(0, "in", [1, 2, 7]), (3, "range", (0, HI))]
    assert 0 < _check(idx, cols, None, _QUERIES[:3], 10, where, "offset 1000") < n
    s, r, _ = idx.search_batch_where(_QUERIES[:1], 10, where)
    assert r.min() >= 1000
    assert idx.count_where(where) == int(where_mask(cols, where, n).sum())
    idx.release()


def test_oracle_anchor(gpu):
    n = 3 * _strip() + 37
    m, cols = _corpus(n)
    idx = _index(m, cols)
    where = [(0, "not in", [0, TOP]), (1, "range", (0, HI)), (3, "no_bits", 4)]
    S = np.flatnonzero(where_mask(cols, where, n))
    assert 100 < len(S) < n
    q = _QUERIES[0]
    for k in (1, 100, len(S)):
        got, matched = idx.search_where(q, k, where)
        assert matched == len(S)
        exp = oracle.cpu_search(m[S], q, k)
        truth = m[S].astype(np.float64) @ q.astype(np.float64)
        got_rows = np.array([row for _, row in got], dtype=np.int64)
        pos = np.searchsorted(S, got_rows)
        assert np.array_equal(S[np.minimum(pos, len(S) - 1)], got_rows), "a row outside the matching set"
        assert_topk_parity([s for s, _ in got], pos, [s for s, _ in exp], [p for _, p in exp], truth64=truth,
                           label=f"oracle k={k}", score_atol=TOL_F32)
    idx.release()


def test_planted_patterns(gpu):
    from svs_amd import DeviceIndex
    r = _strip()
    n = 3 * r + 37
    m, _ = _corpus(n)
    idx = DeviceIndex(m)
    patterns = {"row 0": [0], "last row": [n - 1], "every row": np.arange(n),
                "one per strip": [s * r + (s * 677 + 5) % min(r, n - s * r) for s in range(4)],
                "last strip": np.arange(3 * r, n)}
    for name, hits in patterns.items():
        planted = np.full(n, 3, dtype=np.uint32)                 # 3: below the range, without the bit
        planted[np.asarray(hits)] = 0x50
        idx.set_column(1, planted)
        cols = {1: planted}
        for where in ([(1, "range", (0x40, 0x5F))], [(1, "any_bits", 0x10)], [(1, "range", (4, TOP)), (1, "any_bits", 0x40)]):
            for nq, k in ((1, 10), (3, len(hits)), (3, len(hits) + 5)):
                assert _check(idx, cols, None, _QUERIES[:nq], k, where, f"{name} {where}") == len(hits)
        got = idx.search_batch_where(_QUERIES[:1], n, [(1, "any_bits", 0x10)])[1]
        assert sorted(got[0].tolist()) == sorted(int(h) for h in hits)
    idx.release()


# ---- the raw entry: limits, count-only calls, errors ----------------------------------------------------------------
S_SENT, R_SENT, C_SENT, M_SENT = np.float32(-7.5), -77, -777, -7777


def _term(column=0, op=0, negate=0, a=0, b=0, members=None, nset=None, keep=None):
    from svs_amd import _native
    t = _native.WhereTerm()
    t.column, t.op, t.negate, t.a, t.b = column, op, negate, a, b
    arr = None if members is None else np.ascontiguousarray(members, dtype=np.uint32)
    if keep is not None and arr is not None:
        keep.append(arr)
    t.set = arr.ctypes.data if arr is not None and len(arr) else None
    t.nset = (len(arr) if arr is not None else 0) if nset is None else nset
    return t


class _Raw:
    """svs_index_search_where with sentinel-filled outputs."""

    def __init__(self, idx, nq=2, k=4):
        from svs_amd import _native
        self.lib, self.native, self.h = _native.load(), _native, idx._handle()
        self.q = np.ascontiguousarray(_unit_rows(np.random.default_rng(8), max(nq, 1), idx.d))
        self.s = np.full((max(nq, 1), max(k, 1)), S_SENT, dtype=np.float32)
        self.r = np.full((max(nq, 1), max(k, 1)), R_SENT, dtype=np.int64)
        self.keep = []

    def call(self, nq, d, k, terms, nterms=None, q=True, s=True, r=True, count=True, matched=True):
        arr = (self.native.WhereTerm * max(len(terms), 1))(*terms) if terms is not None else None
        self.s[:], self.r[:] = S_SENT, R_SENT
        self.count, self.matched = C.c_int32(C_SENT), C.c_int64(M_SENT)
        rc = self.lib.svs_index_search_where(
            self.h, self.q.ctypes.data if q else None, nq, d, k, arr, (len(terms) if terms is not None else 0) if nterms is None else nterms,
            self.s.ctypes.data if s else None, self.r.ctypes.data if r else None, C.byref(self.count) if count else None,
            C.byref(self.matched) if matched else None)
        self.launches = self.native.last_launches()
        return rc

    def untouched(self):
        return bool((self.s == S_SENT).all() and (self.r == R_SENT).all())


def test_limits_on_members_and_terms(gpu):
    from svs_amd import _native
    n = 65
    m, cols = _corpus(n)
    idx = _index(m, cols)
    low, high = [2] + list(range(1000, 1511)), [7] + list(range(3000, 3511))          # 512 + 512 distinct members
    where = [(0, "in", low), (1, "in", high)]
    want = int((np.isin(cols[0], low) & np.isin(cols[1], high)).sum())
    assert _check(idx, cols, None, _QUERIES[:2], 10, where, "1,024 members over two terms") == want
    assert idx.count_where([(0, "in", low + low), (1, "not in", high)]) == int((np.isin(cols[0], low) & ~np.isin(cols[1], high)).sum())
    with pytest.raises(ValueError):
        idx.search_batch_where(_QUERIES, 3, [(0, "in", low), (1, "in", high + [9])])   # 1,025
    with pytest.raises(ValueError):
        idx.count_where([(0, "range", (0, 1))] * 5)
    raw = _Raw(idx)

    def failed(rc, want_rc):
        assert rc == want_rc, (rc, want_rc, _native.last_error())
        assert raw.untouched() and raw.count.value == C_SENT and raw.matched.value == M_SENT and raw.launches == []

    keep = []
    failed(raw.call(2, D, 4, [_term(0, 0, members=low, keep=keep), _term(1, 0, members=high + [9], keep=keep)]), _native.SVS_ERR_UNSUPPORTED)
    failed(raw.call(2, D, 0, [_term(0, 0, members=range(1025), keep=keep)]), _native.SVS_ERR_UNSUPPORTED)
    failed(raw.call(2, D, 4, [_term(0, 1, a=0, b=TOP)] * 5), _native.SVS_ERR_UNSUPPORTED)
    # repeats do not count, and only IN terms have members
    assert raw.call(2, D, 4, [_term(0, 0, members=low + low, keep=keep), _term(1, 0, members=high, keep=keep),
                              _term(3, 1, a=0, b=TOP, members=range(2000), nset=2000, keep=keep)]) == 0
    assert raw.matched.value == want
    idx.release()


def test_count_only_calls(gpu):
    n = _strip() + 1
    m, cols = _corpus(n)
    idx = _index(m, cols)
    raw = _Raw(idx)
    keep = []
    terms = [_term(0, 0, members=[7, 2], keep=keep), _term(1, 3, negate=1, a=1)]
    want = int(where_mask(cols, [(0, "in", [2, 7]), (1, "not all_bits", 1)], n).sum())
    assert 0 < want < n
    for nq, k in ((2, 0), (2, -3), (0, 4)):                      # count only: the count launch alone
        assert raw.call(nq, D, k, terms) == 0
        assert raw.matched.value == want and raw.count.value == 0 and raw.untouched()
        assert _names(raw.launches) == ["where_count_kernel"], raw.launches
        assert raw.call(nq, D, k, terms, s=False, r=False, q=nq > 0) == 0 and raw.matched.value == want
        assert raw.call(nq, D, k, terms, matched=False) == 0     # nobody to tell the count: nothing launched
        assert raw.count.value == 0 and raw.untouched() and raw.launches == []
    from svs_amd import _native
    assert idx.count_where([(0, "in", [2, 7]), (1, "not all_bits", 1)]) == want
    assert _names(_native.last_launches()) == ["where_count_kernel"]
    assert idx.count_where([]) == n and _names(_native.last_launches()) == ["where_count_kernel"]
    # no term: every live row; the empty set takes no short-cut on the host: the count pass finds it
    assert raw.call(2, D, 4, None) == 0 and raw.matched.value == n and raw.count.value == 4
    assert raw.call(2, D, 4, [_term(0, 0)]) == 0 and raw.matched.value == 0 and raw.count.value == 0 and raw.untouched()
    assert _names(raw.launches) == ["where_count_kernel"]
    # a full call through the same harness: entries past the count stay untouched
    planted = np.zeros(n, dtype=np.uint32)
    planted[[3, n - 1]] = 9
    idx.set_column(2, planted)
    assert raw.call(2, D, 4, [_term(2, 1, a=9, b=9)]) == 0 and raw.count.value == 2 and raw.matched.value == 2
    assert (raw.s[:, 2:] == S_SENT).all() and (raw.r[:, 2:] == R_SENT).all()
    assert sorted(raw.r[0, :2].tolist()) == [3, n - 1]
    assert raw.call(2, D, 4, [_term(2, 1, a=9, b=9)], count=False) == 0 and raw.matched.value == 2
    idx.release()


def test_errors_write_nothing_and_launch_nothing(gpu):
    from svs_amd import DeviceIndex, _native
    n = 65
    m, cols = _corpus(n)
    idx = _index(m, cols)
    raw = _Raw(idx)
    keep = []
    ok = [_term(0, 0, members=[1], keep=keep)]
    INV = _native.SVS_ERR_INVALID

    def failed(rc, want):
        assert rc == want, (rc, want, _native.last_error())
        assert raw.untouched() and raw.count.value == C_SENT and raw.matched.value == M_SENT and raw.launches == []

    failed(raw.call(2, D + 1, 4, ok), _native.SVS_ERR_SHAPE)
    failed(raw.call(-1, D, 4, ok), INV)
    failed(raw.call(2, D, 4, ok, nterms=-1), INV)
    failed(raw.call(2, D, 4, None, nterms=2), INV)               # null terms
    failed(raw.call(2, D, 4, [_term(4, 1, a=0, b=1)]), INV)      # a column outside the range
    failed(raw.call(2, D, 4, [_term(-1, 1, a=0, b=1)]), INV)
    failed(raw.call(2, D, 4, [_term(0, 4, a=1)]), INV)           # an unknown op
    failed(raw.call(2, D, 4, [_term(0, -1, a=1)]), INV)
    failed(raw.call(2, D, 4, [_term(0, 2, negate=2, a=1)]), INV) # negate not 0 or 1
    failed(raw.call(2, D, 4, [_term(0, 2, negate=-1, a=1)]), INV)
    failed(raw.call(2, D, 4, [_term(0, 0, members=[1], nset=-1, keep=keep)]), INV)
    failed(raw.call(2, D, 4, [_term(0, 0, members=None, nset=3)]), INV)    # a null set with nset > 0
    failed(raw.call(2, D, 4, ok + [_term(1, 0, members=None, nset=1)]), INV)
    failed(raw.call(2, D, 4, ok, q=False), INV)
    failed(raw.call(2, D, 4, ok, s=False), INV)
    failed(raw.call(2, D, 4, ok, r=False), INV)
    failed(raw.call(2, D, 0, [_term(0, 4, a=1)]), INV)           # ... also when the call would only count
    # set / nset are ignored on the other ops
    assert raw.call(2, D, 4, [_term(0, 1, a=0, b=TOP, members=None, nset=-5)]) == 0 and raw.matched.value == n
    with pytest.raises(ValueError):
        idx.search_batch_where(_QUERIES, 3, [(0, "in", [-1])])
    with pytest.raises(ValueError):
        idx.search_where(_QUERIES, 3, [])                        # a 2-D query
    idx.release()

    empty = DeviceIndex.empty(D)
    raw = _Raw(empty)
    failed(raw.call(2, D, 4, ok), _native.SVS_ERR_SHAPE)
    empty.release()

    # rows of more than 16 KiB: no gather kernel takes them; counting still works
    wide = DeviceIndex(_unit_rows(np.random.default_rng(2), 8, 4100))
    wide.set_column(3, [1, 2, 1, 2, 1, 2, 1, 2])
    raw = _Raw(wide)
    failed(raw.call(2, 4100, 4, [_term(3, 1, a=1, b=1)]), _native.SVS_ERR_UNSUPPORTED)
    assert raw.call(2, 4100, 0, [_term(3, 1, a=1, b=1)]) == 0 and raw.matched.value == 4
    wide.release()

"""CPU: the row-list builder of the filtered searches (live_rows_ascending in svs_amd/csrc/svs_amd.hip, through
svs_internal_live_rows).

svs_index_search_rows builds its one device list with it, svs_index_search_segments the list of every segment: the
distinct live listed rows as local u32 rows, ascending.  An ascending list is filtered as it stands, any other is sorted
and deduplicated first; tombstoned rows drop out on both paths.  The model is ``np.unique(rows)`` without the dead
rows, compared as arrays."""
import numpy as np
import pytest

from svs_amd import _native

GUARD = 0xDEADBEEF


def live_rows(rows, n, dead=(), row_offset=0, cap=None):
    """(return value, out array) of svs_internal_live_rows; ``rows`` are GLOBAL rows, ``dead`` local ones."""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    flags[np.asarray(dead, dtype=np.int64)] = 1
    cap = len(rows) if cap is None else cap
    out = np.full(max(cap, len(rows), 1), GUARD, dtype=np.uint32)
    m = int(_native.load().svs_internal_live_rows(rows.ctypes.data, len(rows), row_offset, n, flags.ctypes.data, out.ctypes.data, cap))
    return m, out


def expected(rows, dead=(), row_offset=0):
    local = np.unique(np.asarray(rows, dtype=np.int64)) - row_offset
    return local[~np.isin(local, np.asarray(dead, dtype=np.int64))].astype(np.uint32)


def check(rows, n, dead=(), row_offset=0):
    m, out = live_rows(rows, n, dead, row_offset)
    assert m >= 0, _native.last_error()
    exp = expected(rows, dead, row_offset)
    np.testing.assert_array_equal(out[:m], exp)
    assert np.all(out[m:] == GUARD)   # (nothing is written behind the m rows)
    return m


def test_ascending_shuffled_and_repeated_lists_give_the_same_rows():
    rng = np.random.default_rng(5)
    n = 5000
    asc = np.sort(rng.choice(n, 1700, replace=False))
    dead = rng.choice(n, 900, replace=False)
    m = check(asc, n, dead)                                   # the fast path
    assert 0 < m < len(asc)
    assert check(rng.permutation(asc), n, dead) == m          # sort + unique
    assert check(rng.permutation(np.repeat(asc, 2)), n, dead) == m
    assert check(rng.permutation(np.repeat(asc, 3)), n, dead) == m
    assert check(np.repeat(asc, 3), n, dead) == m             # non-decreasing is not ascending: repeats must go


def test_smallest_lists():
    n = 300
    assert check([n - 1, 0], n) == 2
    assert check([17], n) == 1
    assert check([17], n, dead=[17]) == 0
    assert check([], n) == 0
    assert check([0], 1) == 1


def test_dead_rows_first_last_alternating_and_all():
    rng = np.random.default_rng(6)
    n = 1000
    rows = np.arange(100, 900)
    for listed in (rows, rng.permutation(rows)):
        assert check(listed, n, dead=rows) == 0                               # every listed row dead
        assert check(listed, n, dead=rows[:50]) == len(rows) - 50             # first
        assert check(listed, n, dead=rows[-50:]) == len(rows) - 50            # last
        assert check(listed, n, dead=rows[::2]) == len(rows) // 2             # alternating
        assert check(listed, n, dead=np.concatenate([rows[:1], rows[-1:]])) == len(rows) - 2


def test_row_offset_is_subtracted_in_64_bits():
    rng = np.random.default_rng(7)
    lo, n = 10 ** 12, 4000
    rows = lo + rng.choice(n, 1500, replace=False)
    dead = rng.choice(n, 400, replace=False)
    assert check(np.sort(rows), n, dead, row_offset=lo) == check(rows, n, dead, row_offset=lo) > 0
    assert check([lo + n - 1, lo], n, row_offset=lo) == 2


def test_more_than_65536_distinct_rows():
    rng = np.random.default_rng(8)
    n = 70000
    rows = rng.choice(n, 66000, replace=False)
    dead = rng.choice(n, 5000, replace=False)
    m = check(rows, n, dead)
    assert m == check(np.sort(rows), n, dead) > 1 << 15
    assert check(rows, n) == 66000


@pytest.mark.parametrize("case", ["below", "at_end", "cap", "null"])
def test_errors_leave_out_untouched(case):
    lo, n = 1000, 50
    rows = {"below": [lo + 3, lo - 1, lo + 4], "at_end": [lo + 3, lo + n], "cap": [lo + 1, lo + 2, lo + 3], "null": [lo + 1, lo + 2]}[case]
    if case == "null":
        flags = np.zeros(n, dtype=np.uint8)
        out = np.full(4, GUARD, dtype=np.uint32)
        rc = _native.load().svs_internal_live_rows(None, 2, lo, n, flags.ctypes.data, out.ctypes.data, 4)
    else:
        rc, out = live_rows(rows, n, row_offset=lo, cap=2 if case == "cap" else None)
    assert rc == _native.SVS_ERR_INVALID
    assert np.all(out == GUARD)

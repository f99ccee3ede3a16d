"""GPU: the u32 columns beside the rows (svs_index_set_column / svs_index_get_column) -- round trips, what they cost in
HBM, column 0 being the label column, growth, tombstones and compaction -- each seen through ``column()`` and through
``search_where`` (held against ``search_batch_within`` over the rows the numpy model selects)."""
import numpy as np
import pytest

from where_model import where_mask

pytestmark = pytest.mark.gpu

D = 64
HI, TOP = 0x80000000, 0xFFFFFFFF
VALUES = np.array([0, 1, 2, 7, HI, TOP], dtype=np.uint32)
WHERE = [(0, "in", [1, 2, 7, TOP]), (1, "not range", (1, 2)), (3, "no_bits", 4)]


def _strip():
    from svs_amd import _native
    return int(_native.load().svs_internal_labels_strip())


def _unit_rows(rng, n, d=D):
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


_QUERIES = _unit_rows(np.random.default_rng(6), 3)


def _corpus(n, seed=0):
    rng = np.random.default_rng(3000 + n + seed)
    return _unit_rows(rng, n), {c: VALUES[rng.integers(0, len(VALUES), n)] for c in (0, 1, 3)}


def _same_as_within(idx, cols, dead, where, k, tag):
    sel = where_mask(cols, where, idx.n) & (~dead if dead is not None else True)
    rows = np.flatnonzero(sel) + idx.row_offset
    s, r, matched = idx.search_batch_where(_QUERIES, k, where)
    es, er = idx.search_batch_within(_QUERIES, k, rows)
    assert matched == len(rows), (tag, matched, len(rows))
    assert s.tobytes() == es.tobytes() and np.array_equal(r, er), tag
    return matched


def test_round_trip_partial_ranges_and_cost(gpu):
    from svs_amd import DeviceIndex, _native
    n = _strip() + 1
    m, cols = _corpus(n)
    idx = DeviceIndex(m, row_offset=500)
    base = idx.hbm_bytes
    for c in range(4):
        assert not idx.column(c).any() and idx.column(c).shape == (n,) and idx.column(c).dtype == np.uint32
    idx.set_column(2, [])                                        # nothing: no column is allocated by reads or empty writes
    assert idx.hbm_bytes == base
    for c in (3, 1, 0):
        before = idx.hbm_bytes
        idx.set_column(c, cols[c][40:90], row0=540)              # the first write: everything else stays 0
        assert idx.hbm_bytes >= before + 4 * n                   # one u32 per row, counted
        want = np.zeros(n, dtype=np.uint32)
        want[40:90] = cols[c][40:90]
        assert np.array_equal(idx.column(c), want)
        first = idx.hbm_bytes
        idx.set_column(c, cols[c])                               # (row0=None: from the index's first row, 500)
        assert idx.hbm_bytes == first and np.array_equal(idx.column(c), cols[c])
        assert np.array_equal(idx.column(c, 500 + 5, 7), cols[c][5:12]) and idx.column(c, 505, 0).shape == (0,)
        idx.set_column(c, [TOP], row0=500 + n - 1)
        cols[c] = cols[c].copy()
        cols[c][n - 1] = TOP
        assert int(idx.column(c, 500 + n - 1, 1)[0]) == TOP and np.array_equal(idx.column(c), cols[c])
    after = idx.hbm_bytes
    assert after >= base + 3 * 4 * n and not idx.column(2).any()
    idx.set_column(0, cols[0])                                   # a second write allocates nothing
    assert idx.hbm_bytes == after
    # the others are untouched by a write to one
    idx.set_column(1, np.zeros(10, dtype=np.uint32), row0=500)
    cols[1] = cols[1].copy()
    cols[1][:10] = 0
    for c in (0, 1, 3):
        assert np.array_equal(idx.column(c), cols[c])
    assert _same_as_within(idx, cols, None, WHERE, 10, "offset 500") > 0
    for bad in ((499, 2), (500 + n - 1, 2), (500 + n + 1, 1)):
        with pytest.raises(ValueError):
            idx.set_column(1, np.zeros(bad[1], dtype=np.uint32), row0=bad[0])
        with pytest.raises(ValueError):
            idx.column(1, bad[0], bad[1])
    for bad in ([-1], [2 ** 32], [1.5]):
        with pytest.raises(ValueError):
            idx.set_column(1, bad)
    with pytest.raises(ValueError):
        idx.column(1, 500, -1)
    # the raw entries: the column number, a negative count, null buffers; an empty range is fine whatever the pointers
    lib, h, buf = _native.load(), idx._handle(), np.full(4, 0xABCD, dtype=np.uint32)
    INV = _native.SVS_ERR_INVALID
    for c in (-1, 4):
        assert lib.svs_index_set_column(h, c, 500, 4, buf.ctypes.data) == INV and lib.svs_index_get_column(h, c, 500, 4, buf.ctypes.data) == INV
    assert lib.svs_index_set_column(h, 1, 500, -1, buf.ctypes.data) == INV and lib.svs_index_set_column(h, 1, 500, 3, None) == INV
    assert lib.svs_index_get_column(h, 1, 500, 3, None) == INV
    assert lib.svs_index_get_column(h, 1, 500 + n - 2, 4, buf.ctypes.data) == INV and (buf == 0xABCD).all()
    assert lib.svs_index_set_column(h, 2, 500, 0, None) == 0 and lib.svs_index_get_column(h, 2, 500, 0, None) == 0
    assert lib.svs_index_set_column(None, 1, 0, 1, buf.ctypes.data) == INV
    assert idx.hbm_bytes == after and np.array_equal(idx.column(1), cols[1])
    idx.release()


def test_column_0_is_the_label_column(gpu):
    from svs_amd import DeviceIndex
    n = 65
    m, cols = _corpus(n)
    idx = DeviceIndex(m)
    base = idx.hbm_bytes
    idx.set_labels(cols[0])
    one = idx.hbm_bytes
    assert one >= base + 4 * n and np.array_equal(idx.column(0), cols[0])
    idx.set_column(0, cols[1][:20], row0=10)
    want = cols[0].copy()
    want[10:30] = cols[1][:20]
    assert idx.hbm_bytes == one and np.array_equal(idx.labels(), want) and np.array_equal(idx.column(0), want)
    idx.set_labels([9], row0=n - 1)
    want[n - 1] = 9
    assert np.array_equal(idx.column(0), want)
    s, r, matched = idx.search_batch_labeled(_QUERIES, n, [9, 7])
    ws, wr, wmatched = idx.search_batch_where(_QUERIES, n, [(0, "in", [7, 9])])
    assert matched == wmatched == int(np.isin(want, [7, 9]).sum()) and s.tobytes() == ws.tobytes() and np.array_equal(r, wr)
    idx.release()
    other = DeviceIndex(m)                                       # and the other way round: set_column(0) first
    other.set_column(0, cols[0])
    assert np.array_equal(other.labels(), cols[0]) and other.hbm_bytes == one
    other.release()


def test_growth_keeps_columns_and_new_rows_read_zero(gpu):
    from svs_amd import DeviceIndex
    r = _strip()
    m, _ = _corpus(3 * r + 37)
    old = {1: np.array([1, 2, 7, TOP] * 25, dtype=np.uint32), 3: np.array([HI, 1, 1, 2, 7] * 20, dtype=np.uint32)}   # 100 rows, no 0
    idx = DeviceIndex(m[:100])
    for c, v in old.items():
        idx.set_column(c, v)
    two = idx.hbm_bytes
    idx.append(m[100:100 + r + 5])                               # past the capacity: the buffers are reallocated
    n = idx.n
    cols = {c: np.concatenate([v, np.zeros(n - 100, dtype=np.uint32)]) for c, v in old.items()}
    for c in range(4):
        assert np.array_equal(idx.column(c), cols.get(c, np.zeros(n, dtype=np.uint32)))
    # search_where sees both: the old rows by their values, the new rows as 0
    s, rows, matched = idx.search_batch_where(_QUERIES[:1], n, [(1, "in", [0]), (3, "range", (0, 0))])
    assert matched == n - 100 and sorted(rows[0].tolist()) == list(range(100, n))
    s, rows, matched = idx.search_batch_where(_QUERIES[:1], n, [(1, "not in", [0])])
    assert matched == 100 and sorted(rows[0].tolist()) == list(range(100))
    for where in ([(1, "in", [7, 0])], [(3, "any_bits", HI | 2), (1, "not range", (2, 7))], [(1, "no_bits", 1), (0, "in", [0])]):
        assert 0 < _same_as_within(idx, cols, None, where, 10, f"grown {where}") < n
    fresh = VALUES[np.random.default_rng(3).integers(0, len(VALUES), n - 100)]
    idx.set_column(3, fresh, row0=100)
    cols[3][100:] = fresh
    assert np.array_equal(idx.column(3), cols[3]) and np.array_equal(idx.column(1), cols[1])
    _same_as_within(idx, cols, None, [(3, "not in", [0, 1]), (1, "range", (0, 7))], 10, "grown and set")
    grown = idx.hbm_bytes
    idx.reserve(2 * n)                                           # an explicit reserve carries the columns along
    for c in (1, 3):
        assert np.array_equal(idx.column(c), cols[c])
    _same_as_within(idx, cols, None, [(3, "not in", [0, 1]), (1, "range", (0, 7))], 10, "reserved")
    # the never-set columns stayed unallocated: two columns' worth of bytes, not four
    bare = DeviceIndex(m[:100])
    bare.append(m[100:100 + r + 5])
    bare.reserve(2 * n)
    assert idx.hbm_bytes - bare.hbm_bytes == 2 * 4 * ((2 * n + 3) // 4 * 4) and grown > two
    bare.release()
    idx.release()


def test_tombstones_and_compaction(gpu):
    from svs_amd import DeviceIndex
    r = _strip()
    n = 3 * r + 37
    m, cols = _corpus(n)
    for dtype in ("f32", "fp8"):
        idx = DeviceIndex(m, dtype=dtype, row_offset=10)
        for c, v in cols.items():
            idx.set_column(c, v)
        three = idx.hbm_bytes
        full = _same_as_within(idx, cols, None, WHERE, 10, "before masking")
        hits = np.flatnonzero(where_mask(cols, WHERE, n))
        dead = np.zeros(n, dtype=bool)
        dead[np.random.default_rng(9).permutation(n)[:n // 4]] = True     # about a quarter of the rows
        dead[[0, n - 1, r, hits[0]]] = True                               # strip edges, and a row that matches
        idx.mask_rows(np.flatnonzero(dead) + 10)
        for c in range(4):                                               # masking does not touch the columns: they are still read back
            assert np.array_equal(idx.column(c), cols.get(c, np.zeros(n, dtype=np.uint32)))
        still = _same_as_within(idx, cols, dead, WHERE, 10, "masked")
        assert still == full - int(dead[hits].sum()) < full
        got = idx.search_batch_where(_QUERIES[:1], n, WHERE)
        assert not set(got[1][0].tolist()) & set((np.flatnonzero(dead) + 10).tolist())
        idx.set_column(1, [TOP], row0=10)                                # a tombstoned row may be written and read
        assert int(idx.column(1, 10, 1)[0]) == TOP
        idx.set_column(1, cols[1][:1], row0=10)
        before = idx.search_batch_where(_QUERIES, n, WHERE)
        old_rows = idx.compact()
        assert idx.n == n - int(dead.sum()) and np.array_equal(old_rows, np.flatnonzero(~dead) + 10)
        new_cols = {c: v[~dead] for c, v in cols.items()}
        for c in range(4):                                               # every column afterwards equals col[live]
            assert np.array_equal(idx.column(c), new_cols.get(c, np.zeros(idx.n, dtype=np.uint32)))
        after = idx.search_batch_where(_QUERIES, n, WHERE)
        assert after[2] == before[2] == still and after[0].tobytes() == before[0].tobytes()
        assert np.array_equal(old_rows[after[1] - 10], before[1])        # the same rows, renumbered by the map
        _same_as_within(idx, new_cols, None, WHERE, 10, f"{dtype} compacted")
        assert idx.hbm_bytes == three                                    # the never-set column is still not there
        # rows appended behind a compaction read 0 in every column, not what the tails held before it
        idx.append(m[:50])
        for c in range(4):
            assert not idx.column(c, 10 + idx.n - 50, 50).any()
        idx.release()


def test_a_never_set_column_stays_unallocated(gpu):
    from svs_amd import DeviceIndex
    n = _strip() + 1
    m, cols = _corpus(n)
    idx = DeviceIndex(m, dtype="f16")
    bare = DeviceIndex(m, dtype="f16")
    dead = np.zeros(n, dtype=bool)
    dead[::7] = True
    for i in (idx, bare):
        i.mask_rows(np.flatnonzero(dead))
    assert idx.hbm_bytes == bare.hbm_bytes
    # an index without any column: every value reads 0, nothing is allocated by searching
    zeros = {}
    assert _same_as_within(idx, zeros, dead, [(1, "in", [0]), (3, "all_bits", 0)], 10, "no column") == n - int(dead.sum())
    assert _same_as_within(idx, zeros, dead, [(2, "any_bits", TOP)], 10, "no column, nothing") == 0
    assert idx.hbm_bytes == bare.hbm_bytes
    idx.set_column(3, cols[3])
    one = idx.hbm_bytes - bare.hbm_bytes
    assert one >= 4 * n
    for i in (idx, bare):
        i.compact()
        i.append(np.vstack([m, m]))                              # growth
    cap_cols = idx.hbm_bytes - bare.hbm_bytes
    assert 4 * idx.n <= cap_cols < 2 * 4 * idx.n                 # still ONE column beside the rows
    assert not idx.column(0).any() and not idx.column(1).any() and not idx.column(2).any()
    assert np.array_equal(idx.column(3)[:n - int(dead.sum())], cols[3][~dead])
    for i in (idx, bare):
        i.release()

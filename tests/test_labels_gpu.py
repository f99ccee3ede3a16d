"""GPU: labelled search (svs_index_search_labeled, labels.h) -- top-k over the live rows whose stored label is in a set,
with the filter run on the device -- and the label column itself (set / get, growth, tombstones, compaction).

The core assertion is the entry's definition: the result equals ``search_batch_within`` over
``flatnonzero(isin(labels, set) & live) + row_offset`` bit for bit (scores, rows, count), ``matched`` equals the numpy
count, and ``svs_internal_last_launches`` names both label kernels and the gather kernel the ``search_rows`` call
took.  One case is also held against ``oracle.cpu_search`` over the matching rows, so that the chain does not hang on
``search_rows`` alone.  Corpus sizes sit around the filter's workgroup strip (``svs_internal_labels_strip``)."""
import ctypes as C

import numpy as np
import pytest

from compare import assert_topk_parity
from oracle import svs_oracle as oracle

pytestmark = pytest.mark.gpu

D = 64
VALUES = np.array([0, 1, 2, 7, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
BIG = [2] + list(range(1000, 1000 + 1023))          # 1,024 labels, of which the corpora carry one
SETS = {"one": [1], "zero": [0], "two": [2, 7], "repeat": [0xFFFFFFFF, 1, 1], "big": BIG, "none": [5]}
TOL_F32 = 2e-6                                       # tests/test_search_within_gpu.py: TOL


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
    """(rows, labels drawn from VALUES) of an n-row corpus, made once."""
    if n not in _CORPORA:
        rng = np.random.default_rng(1000 + n)
        _CORPORA[n] = (_unit_rows(rng, n), VALUES[rng.integers(0, len(VALUES), n)])
    return _CORPORA[n]


def _names(launches):
    return [rec[0] for rec in launches]


def _check(idx, labels, dead, q, k, label_set, tag):
    """One labelled call against search_batch_within over the rows numpy selects; returns matched."""
    from svs_amd import _native
    lo = idx.row_offset
    sel = np.isin(labels, np.asarray(label_set, dtype=np.uint32))
    if dead is not None:
        sel &= ~dead
    rows = np.flatnonzero(sel) + lo
    s, r, matched = idx.search_batch_labeled(q, k, label_set)
    ours = _native.last_launches()
    es, er = idx.search_batch_within(q, k, rows)
    theirs = _native.last_launches()
    count = min(max(k, 0), len(rows))
    assert matched == len(rows), (tag, matched, len(rows))
    assert s.shape == es.shape == (len(q), count) and r.shape == er.shape, (tag, s.shape, es.shape)
    assert s.tobytes() == es.tobytes(), f"{tag}: score bits differ"
    assert np.array_equal(r, er), f"{tag}: rows differ"
    if count:
        assert "label_count_kernel" in _names(ours) and "label_write_kernel" in _names(ours), (tag, ours)
        gather = [rec for rec in ours if rec[0].startswith("gather_scores_kernel")]
        assert gather and gather == [rec for rec in theirs if rec[0].startswith("gather_scores_kernel")], (tag, ours, theirs)
    else:
        assert _names(ours) == ["label_count_kernel"], (tag, ours)
    return matched


def _sweep(idx, labels, dead, tag, sets=SETS, nqs=(1, 3)):
    for name, label_set in sets.items():
        m = int((np.isin(labels, np.asarray(label_set, dtype=np.uint32)) & (~dead if dead is not None else True)).sum())
        for nq in nqs:
            for k in sorted({1, 10, max(m, 1), m + 5}):
                _check(idx, labels, dead, _QUERIES[:nq], k, label_set, f"{tag} set={name} nq={nq} k={k}")


def _sizes():
    r = _strip()
    return [1, 63, 65, r - 1, r + 1, 3 * r + 37]


@pytest.mark.parametrize("size", range(6))
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_equals_search_within_over_the_matching_rows(gpu, dtype, size):
    from svs_amd import DeviceIndex
    n = _sizes()[size]
    m, labels = _corpus(n)
    idx = DeviceIndex(m, dtype=dtype)
    before = idx.hbm_bytes
    idx.set_labels(labels)
    assert idx.hbm_bytes >= before + 4 * n                     # the column is counted
    assert np.array_equal(idx.labels(), labels)
    _sweep(idx, labels, None, f"{dtype} n={n}")
    idx.release()


def test_row_offset(gpu):
    from svs_amd import DeviceIndex
    n = _strip() + 1
    m, labels = _corpus(n)
    idx = DeviceIndex(m, row_offset=1000)
    idx.set_labels(labels)                                      # (row0=None: from the index's first row, 1000)
    assert np.array_equal(idx.labels(1000 + 5, 7), labels[5:12])
    _sweep(idx, labels, None, "offset 1000")
    s, r, _ = idx.search_batch_labeled(_QUERIES[:1], 10, [1])
    assert r.min() >= 1000
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
        labels = np.zeros(n, dtype=np.uint32)
        labels[np.asarray(hits)] = 7
        idx.set_labels(labels)
        assert _check(idx, labels, None, _QUERIES[:1], 10, [7], name) == len(hits)
        _sweep(idx, labels, None, name, sets={"seven": [7], "seven and more": [3, 7, 9]}, nqs=(3,))
    idx.release()


def test_oracle_anchor(gpu):
    from svs_amd import DeviceIndex
    n = 3 * _strip() + 37
    m, labels = _corpus(n)
    idx = DeviceIndex(m)
    idx.set_labels(labels)
    S = np.flatnonzero(np.isin(labels, [2, 7]))
    q = _QUERIES[0]
    for k in (1, 100, len(S)):
        got, matched = idx.search_labeled(q, k, [2, 7])
        assert matched == len(S)
        exp = oracle.cpu_search(m[S], q, k)
        truth = m[S].astype(np.float64) @ q.astype(np.float64)
        got_rows = np.array([row for _, row in got], dtype=np.int64)
        pos = np.searchsorted(S, got_rows)
        assert np.array_equal(S[np.minimum(pos, len(S) - 1)], got_rows), "a row outside the matching set"
        assert_topk_parity([s for s, _ in got], pos, [s for s, _ in exp], [p for _, p in exp], truth64=truth,
                           label=f"oracle k={k}", score_atol=TOL_F32)
    idx.release()


def test_tombstones_and_compaction(gpu):
    from svs_amd import DeviceIndex
    r = _strip()
    n = 3 * r + 37
    m, labels = _corpus(n)
    for dtype in ("f32", "fp8"):
        idx = DeviceIndex(m, dtype=dtype, row_offset=10)
        idx.set_labels(labels)
        full = _check(idx, labels, None, _QUERIES[:1], 10, [2, 7], "before masking")
        hits = np.flatnonzero(np.isin(labels, [2, 7]))
        gone = hits[::3]
        dead = np.zeros(n, dtype=bool)
        dead[gone] = True
        dead[[0, n - 1, r]] = True                               # and rows of other labels, at strip edges
        idx.mask_rows(np.flatnonzero(dead) + 10)
        assert np.array_equal(idx.labels(), labels)              # masking does not touch the column
        still = _check(idx, labels, dead, _QUERIES[:1], 10, [2, 7], "masked")
        assert still == full - int(dead[hits].sum())
        _sweep(idx, labels, dead, f"{dtype} masked")
        got = idx.search_batch_labeled(_QUERIES[:1], n, [2, 7])[1]
        assert not set(got[0].tolist()) & set((gone + 10).tolist())
        old_rows = idx.compact()
        new_labels = labels[old_rows - 10]
        assert idx.n == n - int(dead.sum()) and np.array_equal(idx.labels(), new_labels)
        _sweep(idx, new_labels, None, f"{dtype} compacted")
        # rows appended behind a compaction get label 0, not what the tail held before it
        idx.append(m[:50])
        assert not idx.labels(10 + idx.n - 50, 50).any()
        idx.release()


def test_growth_keeps_labels_and_new_rows_read_zero(gpu):
    from svs_amd import DeviceIndex
    r = _strip()
    m, _ = _corpus(3 * r + 37)
    old = np.array([1, 2, 7, 0xFFFFFFFF] * 25, dtype=np.uint32)  # 100 rows, none labelled 0
    idx = DeviceIndex(m[:100])
    idx.set_labels(old)
    idx.append(m[100:100 + r + 5])                               # past the capacity: the buffers are reallocated
    n = idx.n
    labels = np.concatenate([old, np.zeros(n - 100, dtype=np.uint32)])
    assert np.array_equal(idx.labels(), labels)
    s, rows, matched = idx.search_batch_labeled(_QUERIES[:1], n, [0])
    assert matched == n - 100 and sorted(rows[0].tolist()) == list(range(100, n))
    _sweep(idx, labels, None, "grown")
    fresh = VALUES[np.random.default_rng(3).integers(0, len(VALUES), n - 100)]
    idx.set_labels(fresh, row0=100)
    labels[100:] = fresh
    assert np.array_equal(idx.labels(), labels)
    _sweep(idx, labels, None, "grown and labelled")
    idx.reserve(2 * n)                                           # and an explicit reserve carries the column along
    assert np.array_equal(idx.labels(), labels)
    _check(idx, labels, None, _QUERIES[:3], 10, [2, 7], "reserved")
    idx.release()


def test_index_without_a_column(gpu):
    from svs_amd import DeviceIndex
    n = _strip() + 1
    m, _ = _corpus(n)
    idx = DeviceIndex(m, dtype="f16")
    before = idx.hbm_bytes
    dead = np.zeros(n, dtype=bool)
    dead[::7] = True
    idx.mask_rows(np.flatnonzero(dead))
    zeros = np.zeros(n, dtype=np.uint32)
    idx.set_labels([])
    assert not idx.labels().any() and idx.hbm_bytes == before   # an empty set_labels and a read allocate nothing
    _sweep(idx, zeros, dead, "no column", sets={"zero": [0], "five": [5], "zero among others": [9, 0, 3]})
    # {0} is the search over all live rows (held, as everywhere here, against search_batch_within of every live row)
    s, r, matched = idx.search_batch_labeled(_QUERIES, n, [0])
    assert matched == n - int(dead.sum()) and sorted(r[0].tolist()) == np.flatnonzero(~dead).tolist()
    s, r, matched = idx.search_batch_labeled(_QUERIES, 10, [5])
    assert matched == 0 and s.shape == r.shape == (3, 0)
    idx.release()


def test_set_labels_on_a_sub_range(gpu):
    from svs_amd import DeviceIndex
    n = _strip() - 1
    m, labels = _corpus(n)
    idx = DeviceIndex(m)
    idx.set_labels(labels[40:90], row0=40)                       # the first call: everything else stays 0
    want = np.zeros(n, dtype=np.uint32)
    want[40:90] = labels[40:90]
    assert np.array_equal(idx.labels(), want)
    idx.set_labels([0xFFFFFFFF], row0=n - 1)
    idx.set_labels([], row0=3)                                   # nothing
    want[n - 1] = 0xFFFFFFFF
    assert np.array_equal(idx.labels(), want) and int(idx.labels(n - 1, 1)[0]) == 0xFFFFFFFF
    assert idx.labels(5, 0).shape == (0,)
    for bad in ((-1, 2), (n - 1, 2), (n + 1, 1)):
        with pytest.raises(ValueError):
            idx.set_labels(np.zeros(bad[1], dtype=np.uint32), row0=bad[0])
        with pytest.raises(ValueError):
            idx.labels(bad[0], bad[1])
    with pytest.raises(ValueError):
        idx.labels(0, -1)
    with pytest.raises(ValueError):
        idx.set_labels([-1])
    with pytest.raises(ValueError):
        idx.set_labels([2 ** 32])
    # the raw entries: a negative count, null buffers; an empty range is fine whatever the pointers
    from svs_amd import _native
    lib, h, buf = _native.load(), idx._handle(), np.full(4, 0xABCD, dtype=np.uint32)
    assert lib.svs_index_set_labels(h, 0, -1, buf.ctypes.data) == _native.SVS_ERR_INVALID
    assert lib.svs_index_set_labels(h, 0, 3, None) == _native.SVS_ERR_INVALID
    assert lib.svs_index_get_labels(h, 0, 3, None) == _native.SVS_ERR_INVALID
    assert lib.svs_index_get_labels(h, n - 2, 4, buf.ctypes.data) == _native.SVS_ERR_INVALID and (buf == 0xABCD).all()
    assert lib.svs_index_set_labels(h, 0, 0, None) == 0 and lib.svs_index_get_labels(h, 0, 0, None) == 0
    assert lib.svs_index_set_labels(None, 0, 1, buf.ctypes.data) == _native.SVS_ERR_INVALID
    assert np.array_equal(idx.labels(), want)
    _sweep(idx, want, None, "sub-range", sets={"max": [0xFFFFFFFF], "two": [2, 7]}, nqs=(1,))
    idx.release()


# ---- the raw entry: count-only calls, the empty set, errors ---------------------------------------------------------
S_SENT, R_SENT, C_SENT, M_SENT = np.float32(-7.5), -77, -777, -7777


class _Raw:
    """svs_index_search_labeled with sentinel-filled outputs."""

    def __init__(self, idx, nq=2, k=4):
        from svs_amd import _native
        self.lib, self.native, self.h = _native.load(), _native, idx._handle()
        self.q = np.ascontiguousarray(_unit_rows(np.random.default_rng(8), max(nq, 1), idx.d))
        self.s = np.full((max(nq, 1), max(k, 1)), S_SENT, dtype=np.float32)
        self.r = np.full((max(nq, 1), max(k, 1)), R_SENT, dtype=np.int64)

    def call(self, nq, d, k, labels, nlabels=None, q=True, s=True, r=True, count=True, matched=True):
        lab = np.ascontiguousarray(labels, dtype=np.uint32) if labels is not None else None
        self.s[:], self.r[:] = S_SENT, R_SENT
        self.count, self.matched = C.c_int32(C_SENT), C.c_int64(M_SENT)
        rc = self.lib.svs_index_search_labeled(
            self.h, self.q.ctypes.data if q else None, nq, d, k, lab.ctypes.data if lab is not None else None,
            (len(lab) if lab is not None else 0) if nlabels is None else nlabels, self.s.ctypes.data if s else None,
            self.r.ctypes.data if r else None, C.byref(self.count) if count else None, C.byref(self.matched) if matched else None)
        self.launches = self.native.last_launches()
        return rc

    def untouched(self):
        return bool((self.s == S_SENT).all() and (self.r == R_SENT).all())


def test_count_only_and_empty_set_calls(gpu):
    from svs_amd import DeviceIndex
    n = _strip() + 1
    m, labels = _corpus(n)
    idx = DeviceIndex(m)
    idx.set_labels(labels)
    raw = _Raw(idx)
    want = int(np.isin(labels, [2, 7]).sum())
    for nq, k in ((2, 0), (2, -3), (0, 4)):                      # count only: the count launch alone
        assert raw.call(nq, D, k, [7, 2]) == 0
        assert raw.matched.value == want and raw.count.value == 0 and raw.untouched()
        assert _names(raw.launches) == ["label_count_kernel"], raw.launches
        assert raw.call(nq, D, k, [7, 2], s=False, r=False, q=nq > 0) == 0 and raw.matched.value == want
        # nobody to tell the count: nothing launched
        assert raw.call(nq, D, k, [7, 2], matched=False) == 0
        assert raw.count.value == 0 and raw.untouched() and raw.launches == []
    for nq, k in ((2, 4), (2, 0), (0, 4)):                       # the empty set: nothing launched
        assert raw.call(nq, D, k, None) == 0
        assert raw.count.value == 0 and raw.matched.value == 0 and raw.untouched() and raw.launches == []
    assert raw.call(2, D, 4, None, s=False, r=False) == 0 and raw.launches == []
    # a full call through the same harness: entries past the count stay untouched
    assert raw.call(2, D, 4, [0xFFFFFFFF, 1, 1]) == 0
    assert raw.count.value == 4 and raw.matched.value == int(np.isin(labels, [1, 0xFFFFFFFF]).sum()) and not raw.untouched()
    labels2 = np.zeros(n, dtype=np.uint32)
    labels2[[3, n - 1]] = 9
    idx.set_labels(labels2)
    assert raw.call(2, D, 4, [9]) == 0 and raw.count.value == 2 and raw.matched.value == 2
    assert (raw.s[:, 2:] == S_SENT).all() and (raw.r[:, 2:] == R_SENT).all()
    assert sorted(raw.r[0, :2].tolist()) == [3, n - 1]
    # no count pointer at all
    assert raw.call(2, D, 4, [9], count=False) == 0 and raw.matched.value == 2
    idx.release()


def test_errors_write_nothing_and_launch_nothing(gpu):
    from svs_amd import DeviceIndex, _native
    n = 65
    m, labels = _corpus(n)
    idx = DeviceIndex(m)
    idx.set_labels(labels)
    raw = _Raw(idx)

    def failed(rc, want):
        assert rc == want, (rc, want, _native.last_error())
        assert raw.untouched() and raw.count.value == C_SENT and raw.matched.value == M_SENT and raw.launches == []

    failed(raw.call(2, D + 1, 4, [1]), _native.SVS_ERR_SHAPE)
    failed(raw.call(-1, D, 4, [1]), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, [1], nlabels=-1), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, None, nlabels=3), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, [1], q=False), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, [1], s=False), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, [1], r=False), _native.SVS_ERR_INVALID)
    failed(raw.call(2, D, 4, list(range(10, 10 + 1025))), _native.SVS_ERR_UNSUPPORTED)
    failed(raw.call(2, D, 0, list(range(10, 10 + 1025))), _native.SVS_ERR_UNSUPPORTED)
    assert raw.call(2, D, 4, [2] + list(range(10, 10 + 1023)) + [2]) == 0     # 1,025 entries, 1,024 distinct
    assert raw.matched.value == int((labels == 2).sum())
    with pytest.raises(NotImplementedError):
        idx.search_batch_labeled(_QUERIES, 3, list(range(1025)))
    idx.release()

    empty = DeviceIndex.empty(D)
    raw = _Raw(empty)
    failed(raw.call(2, D, 4, [1]), _native.SVS_ERR_SHAPE)
    empty.release()

    # rows of more than 16 KiB: no gather kernel takes them; counting still works
    wide = DeviceIndex(_unit_rows(np.random.default_rng(2), 8, 4100))
    wide.set_labels([1, 2, 1, 2, 1, 2, 1, 2])
    raw = _Raw(wide)
    failed(raw.call(2, 4100, 4, [1]), _native.SVS_ERR_UNSUPPORTED)
    assert raw.call(2, 4100, 0, [1]) == 0 and raw.matched.value == 4
    wide.release()

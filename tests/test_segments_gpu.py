"""GPU: the segmented filtered search (svs_index_search_segments, svs_amd/csrc/segments.h) -- many row lists in one call.

The definition under test: segment s of a call equals ``search_within(queries[seg_query[s]], k, row_lists[s])`` in rows
and score BITS, whatever else is in the call.  So the reference of almost every test here is the library's own
single-list entry point (whose kernels tests/test_gather_kernels_gpu.py and tests/test_search_within_gpu.py pin to f64
and to the oracle), compared without a tolerance; test c compares with the oracle directly.  Every segmented call also
asserts from svs_internal_last_launches what ran: one gather_segments_kernel<DT, T, NC, U> over the live rows of the
segments of up to SORT_CAP rows, one select_segments_kernel, a gather_scores_kernel<..., 1> per larger segment and no
other, nothing over the whole corpus.

A note on test a's sizes: a workgroup of the two shortest row geometries takes B = 4096 or 8192 rows, so the segment of B + 1 rows
is past SORT_CAP there and takes the large route inside the same call; its record is asserted, and a segment of SORT_CAP
rows is added so that the small segments still fill more than one workgroup."""
import threading
import zlib

import numpy as np
import pytest

from compare import assert_topk_parity
from gather_kernel_table import CASES, case_id, choose_ld, rows_per_block, rows_per_wave
from oracle import svs_oracle as oracle
from test_search_within_gpu import TOL

pytestmark = pytest.mark.gpu

SORT_CAP = 4096
FINAL_THREADS = 256


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _unit(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _segments_name(gather_name):
    args = gather_name[gather_name.index("<") + 1:-1].split(", ")
    return f"gather_segments_kernel<{', '.join(args[:4])}>"


def _reference(idx, q, k, rows):
    """(scores f32, rows i64) of search_within, kept as arrays so that the bits can be compared."""
    s, r = idx.search_batch_within(q[None, :], k, rows)
    return s[0].copy(), r[0].copy()


def _live(idx_dead, lo, rows):
    u = np.unique(np.asarray(rows, dtype=np.int64))
    return u if idx_dead is None else u[~idx_dead[u - lo]]


def _assert_launches(idx, lists, gather_single_name, dead=None):
    """What the calling thread's last segmented call ran, against the lists it was given."""
    from svs_amd import _native
    launches = _native.last_launches()
    live = [len(_live(dead, idx.row_offset, r)) for r in lists]
    small = [m for m in live if 1 <= m <= SORT_CAP]
    large = [m for m in live if m > SORT_CAP]
    seg = [rec for rec in launches if rec[0].startswith("gather_segments_kernel")]
    sel = [rec for rec in launches if rec[0].startswith("select_segments_kernel")]
    old = [rec for rec in launches if rec[0].startswith("gather_scores_kernel")]
    want = [(_segments_name(gather_single_name), sum(small), len(small))] if small else []
    assert seg == want, f"launched {launches}, expected {want}"
    assert sel == ([("select_segments_kernel", sum(small), len(small))] if small else []), launches
    assert old == [(gather_single_name, m, 1) for m in large], launches
    assert all(rec[1] != idx.n for rec in launches), f"something ran over the whole corpus: {launches}"


def _assert_equal(got, want, label):
    gs, gr = got
    ws, wr = want
    assert gs.dtype == np.float32 and gr.dtype == np.int64
    assert len(gr) == len(wr), f"{label}: {len(gr)} results, search_within gives {len(wr)}"
    assert np.array_equal(gr, wr), f"{label}: rows differ from search_within, first at rank {np.flatnonzero(gr != wr)[:1]}"
    odd = np.flatnonzero(gs.view(np.uint32) != ws.view(np.uint32))
    assert odd.size == 0, f"{label}: {odd.size} scores differ in bits from search_within, first at rank {odd[0]}: {gs[odd[0]]!r} vs {ws[odd[0]]!r}"


# ---- a. every dtype and geometry: each segment equals search_within, bit for bit ---------------------------------------
def _case_lists(rng, n, w, b):
    """The segments of test a over an n-row corpus, ascending unless said otherwise."""
    def pick(m):
        return np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    sizes = [1, w - 1, w + 1, 0, 2 * w + 1, b + 1] + ([SORT_CAP] if b + 1 > SORT_CAP else [])
    lists = [pick(m) for m in sizes]
    dup = rng.choice(n, w + 3, replace=False).astype(np.int64)
    lists.append(rng.permutation(np.concatenate([dup, dup[:max(w // 2, 2)], dup[:1]])))   # unsorted, with duplicates
    shared = int(rng.integers(1, n - 1))
    for extra in (2, w, 5):                                                               # one row in three segments
        others = pick(extra)
        lists.append(np.unique(np.concatenate([others, [shared]])).astype(np.int64))
    lists.append(np.array([n - 1, 0], dtype=np.int64))                                    # rows 0 and n - 1, descending
    return lists


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_segment_equals_search_within(gpu, case):
    from svs_amd import DeviceIndex
    dtype, d, _, kernel, _ = case
    rng = np.random.default_rng(_seed("segments", case_id(case)))
    w, b = rows_per_wave(kernel), rows_per_block(kernel)
    listed = 1 + w - 1 + w + 1 + 2 * w + 1 + b + 1 + (SORT_CAP if b + 1 > SORT_CAP else 0) + 3 * w + 20
    n = 3 * listed
    idx = DeviceIndex(_unit(rng, n, d), dtype=dtype)
    try:
        assert idx.ld == choose_ld(d, dtype)
        lists = _case_lists(rng, n, w, b)
        nseg = len(lists)
        k = max(len(r) for r in lists)
        # three queries, a non-identity seg_query that repeats
        qs = _unit(rng, 3, d)
        seg_query = [(2 * s + 1) % 3 for s in range(nseg)]
        want = [_reference(idx, qs[j], k, rows) for rows, j in zip(lists, seg_query)]
        got = idx.search_segments(qs, k, lists, seg_query)
        _assert_launches(idx, lists, kernel)
        assert len(got) == nseg
        for s in range(nseg):
            assert len(got[s][1]) == len(np.unique(lists[s])), (case_id(case), s)          # k = the longest: every score is back
            _assert_equal(got[s], want[s], f"{case_id(case)} segment {s} ({len(lists[s])} listed), query {seg_query[s]}")
        # the same segments in another order: the same bits per segment
        perm = rng.permutation(nseg)
        got_p = idx.search_segments(qs, k, [lists[s] for s in perm], [seg_query[s] for s in perm])
        _assert_launches(idx, [lists[s] for s in perm], kernel)
        for i, s in enumerate(perm):
            _assert_equal(got_p[i], want[s], f"{case_id(case)} permuted: segment {s} at place {i}")
        # one query per segment, seg_query=None
        qn = _unit(rng, nseg, d)
        got_n = idx.search_segments(qn, k, lists)
        _assert_launches(idx, lists, kernel)
        for s in range(nseg):
            _assert_equal(got_n[s], _reference(idx, qn[s], k, lists[s]), f"{case_id(case)} seg_query=None: segment {s}")
    finally:
        idx.release()


# ---- b. the selection's edges ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge(gpu):
    """One f32 corpus of d = 1536 for the tests of b (made once): 300 copies of one row among its 13,000."""
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(41)
    m = _unit(rng, 13_000, 1536)
    copies = np.sort(rng.choice(13_000, 300, replace=False))
    m[copies] = m[copies[0]]
    idx = DeviceIndex(m)
    yield {"idx": idx, "copies": copies, "q": _unit(rng, 2, 1536)}
    idx.release()


GATHER_1536 = "gather_scores_kernel<0, 64, 6, 2, 1>"


@pytest.mark.parametrize("k", [1, 10, 5000])
def test_select_edges_in_one_call(edge, k):
    idx, q, rng = edge["idx"], edge["q"], np.random.default_rng(k)
    lists = [np.sort(rng.choice(idx.n, m, replace=False)) for m in (FINAL_THREADS, FINAL_THREADS + 1, SORT_CAP, SORT_CAP + 1)]
    seg_query = [0, 1, 1, 0]
    got = idx.search_segments(q, k, lists, seg_query)
    _assert_launches(idx, lists, GATHER_1536)
    from svs_amd import _native
    assert (GATHER_1536, SORT_CAP + 1, 1) in _native.last_launches()          # the large route, inside the same call
    for s, (rows, j) in enumerate(zip(lists, seg_query)):
        assert len(got[s][1]) == min(k, len(rows))
        _assert_equal(got[s], _reference(idx, q[j], k, rows), f"k={k} segment of {len(rows)} rows")


@pytest.mark.parametrize("others", [50, 700])
def test_ties_come_out_row_descending(edge, others):
    idx, q, copies = edge["idx"], edge["q"], edge["copies"]
    rng = np.random.default_rng(others)
    rest = np.setdiff1d(np.arange(idx.n), copies)
    rows = rng.permutation(np.concatenate([copies, rng.choice(rest, others, replace=False)]))
    lists = [rows, copies[:40], np.sort(rows)[::-1]]
    got = idx.search_segments(q[:1], len(rows), lists, [0, 0, 0])
    _assert_launches(idx, lists, GATHER_1536)
    for s, r in enumerate(lists):
        _assert_equal(got[s], _reference(idx, q[0], len(rows), r), f"ties, segment {s}")
    sc, rr = got[0]
    tied = np.isin(rr, copies)
    assert tied.sum() == 300 and len(np.unique(sc[tied].view(np.uint32))) == 1
    first = int(np.argmax(tied))
    assert tied[first:first + 300].all(), "the copies of one row are not adjacent in the order"
    assert np.array_equal(rr[first:first + 300], np.sort(copies)[::-1]), "equal scores are not ordered row descending"


def test_nan_inf_and_zero_scores_are_ordered_as_search_within_orders_them(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(43)
    d, n = 1536, 2_400
    m = _unit(rng, n, d)
    special = rng.choice(n, 12, replace=False)
    m[special[0], 0] = np.nan
    m[special[1], d - 1] = np.nan
    m[special[2], 0] = np.inf
    m[special[3], d - 1] = np.inf
    m[special[4], 0] = -np.inf
    m[special[5], d - 1] = -np.inf
    m[special[6:9]] = 0.0
    m[special[9:12]] = -0.0
    q = _unit(rng, 2, d)
    q[:, [0, d - 1]] = np.abs(q[:, [0, d - 1]]) + np.float32(1e-3)
    idx = DeviceIndex(m)
    try:
        rest = np.setdiff1d(np.arange(n), special)
        lists = [np.sort(np.concatenate([special, rng.choice(rest, 100, replace=False)])),       # rank emission
                 np.sort(np.concatenate([special, rng.choice(rest, 600, replace=False)])),       # the bitonic network
                 special[6:12]]
        for k in (5, 700):
            got = idx.search_segments(q, k, lists, [0, 1, 1])
            _assert_launches(idx, lists, GATHER_1536)
            for s, (rows, j) in enumerate(zip(lists, [0, 1, 1])):
                _assert_equal(got[s], _reference(idx, q[j], k, rows), f"non-finite, k={k}, segment {s}")
        sc, rr = idx.search_segments(q, 700, lists, [0, 1, 1])[0]
        assert np.isnan(sc[:2]).all() and set(rr[:2]) == set(special[:2])                       # NaN first (largest), row descending
        assert rr[0] > rr[1]
        assert np.isposinf(sc[2:4]).all() and np.isneginf(sc[-2:]).all()
        zero = np.isin(rr, special[6:12])
        assert (sc[zero] == 0).all() and not np.signbit(sc[zero]).any()                         # -0 is folded onto +0
        assert np.array_equal(rr[zero], np.sort(special[6:12])[::-1])
    finally:
        idx.release()


# ---- c. an independent oracle, once per dtype ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_segments_against_the_oracle(gpu, dtype):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(_seed("oracle", dtype))
    n, d, k = 4_000, 1536, 50
    m, qs = _unit(rng, n, d), _unit(rng, 3, d)
    idx = DeviceIndex(m, dtype=dtype)
    try:
        stored = m if dtype == "f32" else idx.stored_rows()
        q_stored = np.stack([idx.stored_query(q) for q in qs])
        lists = [rng.choice(n, 30, replace=False), np.sort(rng.choice(n, 400, replace=False)),
                 np.concatenate([rng.choice(n, 500), rng.choice(n, 300)]), np.array([n - 1, 0, 17])]
        seg_query = [2, 0, 1, 1]
        got = idx.search_segments(qs, k, lists, seg_query)
        for s, (rows, j) in enumerate(zip(lists, seg_query)):
            S = np.unique(rows)
            sub = stored[S]
            exp = oracle.cpu_search(sub, q_stored[j], k)
            truth = sub.astype(np.float64) @ q_stored[j].astype(np.float64)
            sc, rr = got[s]
            assert len(rr) == min(k, len(S))
            pos = np.searchsorted(S, rr)
            assert np.all(pos < len(S)) and np.array_equal(S[np.minimum(pos, len(S) - 1)], rr), f"{dtype} segment {s}: row outside the list"
            err = float(np.max(np.abs(sc.astype(np.float64) - truth[pos])))
            print(f"{dtype} segment {s} ({len(S)} rows): max |score - f64| = {err:.3g}")
            assert_topk_parity(sc.tolist(), pos, [a for a, _ in exp], [p for _, p in exp], truth64=truth,
                               label=f"{dtype} segment {s}", score_atol=TOL[dtype])
            assert err <= TOL[dtype], (dtype, s, err)
    finally:
        idx.release()


# ---- raw calls: sentinels in the outputs --------------------------------------------------------------------------------
S_FILL, R_FILL, C_FILL = np.float32(7.5), -77, -5


def _raw(idx, q, k, lists, seg_query=None, *, nq=None, d=None, nseg=None, begin=None, null=()):
    """svs_index_search_segments itself, outputs pre-filled: (rc, scores (nseg, k), rows (nseg, k), counts)."""
    from svs_amd import _native
    lib = _native.load()
    q = np.ascontiguousarray(q, dtype=np.float32)
    lists = [np.asarray(r, dtype=np.int64).reshape(-1) for r in lists]
    rows = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), dtype=np.int64)
    if begin is None:
        begin = np.concatenate([[0], np.cumsum([len(r) for r in lists])])
    begin = np.ascontiguousarray(begin, dtype=np.int64)
    sq = None if seg_query is None else np.ascontiguousarray(seg_query, dtype=np.int32)
    ns = len(lists) if nseg is None else nseg
    kk = max(k, 1)
    scores = np.full((max(ns, 1), kk), S_FILL, dtype=np.float32)
    out_rows = np.full((max(ns, 1), kk), R_FILL, dtype=np.int64)
    counts = np.full(max(ns, 1), C_FILL, dtype=np.int32)
    h = idx._pinned_handle()
    try:
        rc = lib.svs_index_search_segments(h, q.ctypes.data, q.shape[0] if nq is None else nq, q.shape[1] if d is None else d, k,
                                           rows.ctypes.data, begin.ctypes.data, None if sq is None else sq.ctypes.data, ns,
                                           None if "scores" in null else scores.ctypes.data,
                                           None if "rows" in null else out_rows.ctypes.data,
                                           None if "counts" in null else counts.ctypes.data)
    finally:
        idx._unpin(h)
    return rc, scores, out_rows, counts


def _untouched(res):
    _, s, r, c = res
    return (s == S_FILL).all() and (r == R_FILL).all() and (c == C_FILL).all()


# ---- d. tombstones, row offsets, compaction -----------------------------------------------------------------------------
def test_tombstones_row_offset_and_compaction(gpu):
    from svs_amd import DeviceIndex, _native
    rng = np.random.default_rng(44)
    n, d, off = 3_000, 768, 1_000_000
    m, qs = _unit(rng, n, d), _unit(rng, 2, d)
    kernel = "gather_scores_kernel<0, 64, 3, 4, 1>"
    idx = DeviceIndex(m, row_offset=off)
    try:
        lists = [off + rng.choice(n, s, replace=False) for s in (40, 300, 25, 700, 9)]
        gone = np.unique(np.concatenate([lists[0][::3], lists[1][::2], lists[2], lists[3][:5]]))   # segment 2 entirely dead
        before = idx.search_segments(qs, 50, lists, [0, 1, 0, 1, 1])
        untouched_by_mask = [s for s in range(5) if not np.isin(lists[s], gone).any()]
        idx.mask_rows(gone)
        dead = np.zeros(n, dtype=bool)
        dead[gone - off] = True
        seg_query = [0, 1, 0, 1, 1]
        got = idx.search_segments(qs, 50, lists, seg_query)
        _assert_launches(idx, lists, kernel, dead=dead)
        for s in range(5):
            live = _live(dead, off, lists[s])
            assert len(got[s][1]) == min(50, len(live)) and not np.isin(got[s][1], gone).any() and (got[s][1] >= off).all()
            _assert_equal(got[s], _reference(idx, qs[seg_query[s]], 50, lists[s]), f"tombstones, segment {s}")
        assert len(got[2][1]) == 0
        for s in untouched_by_mask:
            _assert_equal(got[s], before[s], f"segment {s} lists no masked row")
        # entries past a segment's count are not touched; the counts are written for every segment
        rc, sc, rr, cnt = _raw(idx, qs, 50, lists, seg_query)
        assert rc == 0
        for s in range(5):
            c = len(got[s][1])
            assert cnt[s] == c and (sc[s, c:] == S_FILL).all() and (rr[s, c:] == R_FILL).all()
            assert np.array_equal(rr[s, :c], got[s][1]) and np.array_equal(sc[s, :c].view(np.uint32), got[s][0].view(np.uint32))
        # no live listed row anywhere: nothing is launched
        res = _raw(idx, qs, 50, [lists[2], gone[:4]], [0, 1])
        assert res[0] == 0 and res[3].tolist() == [0, 0] and (res[1] == S_FILL).all() and _native.last_launches() == []
        # after compact(), in the new numbering
        old = idx.compact()
        assert idx.n == n - len(gone)
        new_of = {int(o): off + i for i, o in enumerate(old)}
        new_lists = [np.array([new_of[int(r)] for r in rows if int(r) in new_of], dtype=np.int64) for rows in lists]
        got_c = idx.search_segments(qs, 50, new_lists, seg_query)
        _assert_launches(idx, new_lists, kernel)
        for s in range(5):
            _assert_equal(got_c[s], _reference(idx, qs[seg_query[s]], 50, new_lists[s]), f"after compact, segment {s}")
            assert np.array_equal(old[got_c[s][1] - off], got[s][1]), f"after compact, segment {s}: other rows than before"
            assert np.array_equal(got_c[s][0].view(np.uint32), got[s][0].view(np.uint32))
    finally:
        idx.release()


def test_placement_of_segments_around_sort_cap(gpu):
    """Where a segment goes is decided by its LIVE DISTINCT rows, known only once its list is built: segments that list
    more than SORT_CAP rows and are small after all (repeats, tombstones), an unsorted large one, two large ones in a
    call, a small one behind a large one.  At k = 50 against search_within and the launch records; at k >= every live
    count against numpy (the list builder is shared with search_within) and the f64 dot products of the stored rows:
    2e-6, the f32 bound for unit-norm rows."""
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(48)
    n, d, off = 12_000, 768, 1_000_000
    m, qs = _unit(rng, n, d), _unit(rng, 2, d)
    kernel = "gather_scores_kernel<0, 64, 3, 4, 1>"
    gone = rng.choice(n, 3_000, replace=False)
    dead = np.zeros(n, dtype=bool)
    dead[gone] = True
    alive = np.flatnonzero(~dead)
    distinct2 = np.concatenate([rng.choice(alive, 6_500, replace=False), rng.choice(gone, 500, replace=False)])
    lists = [
        rng.choice(rng.choice(n, 3_000, replace=False), 5_000),                                       # small after all: repeats
        rng.permutation(np.concatenate([rng.choice(alive, 3_500, replace=False), rng.choice(gone, 2_500, replace=False)])),   # ... tombstones
        rng.permutation(np.concatenate([distinct2, rng.choice(distinct2, 2_000)])),                   # large, unsorted
        np.sort(rng.choice(alive, 30, replace=False)),                                                # small, behind a large one
        np.sort(rng.choice(alive, 5_000, replace=False)),                                             # large, ascending
        rng.choice(gone, 100, replace=False),                                                         # dead rows only
    ]
    lists = [off + np.asarray(r, dtype=np.int64) for r in lists]
    seg_query = [0, 1, 1, 0, 1, 0]
    live = [_live(dead, off, r) for r in lists]
    assert [len(r) > SORT_CAP for r in lists] == [True, True, True, False, True, False]
    assert [len(u) for u in live][1:] == [3_500, 6_500, 30, 5_000, 0] and 0 < len(live[0]) <= 3_000
    idx = DeviceIndex(m, row_offset=off)
    try:
        idx.mask_rows(off + gone)
        got = idx.search_segments(qs, 50, lists, seg_query)
        _assert_launches(idx, lists, kernel, dead=dead)
        for s in range(6):
            _assert_equal(got[s], _reference(idx, qs[seg_query[s]], 50, lists[s]), f"placement, segment {s}")
        full = idx.search_segments(qs, 8_000, lists, seg_query)
        for s in range(6):
            sc, rr = full[s]
            assert len(rr) == len(live[s]), f"segment {s}: {len(rr)} results for {len(live[s])} distinct live listed rows"
            assert np.array_equal(np.sort(rr), live[s]), f"segment {s}: other rows than the distinct live listed ones"
            tie = sc[:-1] == sc[1:]
            assert np.all((sc[:-1] > sc[1:]) | (tie & (rr[:-1] > rr[1:]))), f"segment {s}: not ordered (score desc, row desc)"
            truth = m[rr - off].astype(np.float64) @ qs[seg_query[s]].astype(np.float64)
            err = float(np.max(np.abs(sc.astype(np.float64) - truth))) if len(rr) else 0.0
            print(f"placement segment {s} ({len(rr)} rows): max |score - f64| = {err:.3g}")
            assert err <= 2e-6, (s, err)
    finally:
        idx.release()


# ---- e. errors ----------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(gpu):
    from svs_amd import DeviceIndex, _native
    rng = np.random.default_rng(45)
    n, d, off = 500, 64, 100
    idx = DeviceIndex(_unit(rng, n, d), row_offset=off)
    q = _unit(rng, 3, d)
    ok = [off + np.arange(5), off + np.arange(10, 40), off + np.array([7, 3]), off + np.arange(100, 104), off + np.array([n - 1])]
    INVALID, SHAPE, UNSUPPORTED = _native.SVS_ERR_INVALID, _native.SVS_ERR_SHAPE, _native.SVS_ERR_UNSUPPORTED
    try:
        bad_seg3 = [r.copy() for r in ok]
        bad_seg3[3][2] = off + n
        low = [r.copy() for r in ok]
        low[0][0] = off - 1
        failing = {
            "d": (SHAPE, _raw(idx, q[:, :d - 1], 5, ok, [0, 1, 2, 0, 1])),
            "nseg < 0": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], nseg=-1)),
            "seg_begin[0]": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], begin=[1, 5, 35, 37, 41, 42])),
            "decreasing": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], begin=[0, 5, 35, 30, 41, 42])),
            "seg_query high": (INVALID, _raw(idx, q, 5, ok, [0, 1, 3, 0, 1])),
            "seg_query low": (INVALID, _raw(idx, q, 5, ok, [0, -1, 2, 0, 1])),
            "no seg_query": (INVALID, _raw(idx, q, 5, ok, None)),
            "row high": (INVALID, _raw(idx, q, 5, bad_seg3, [0, 1, 2, 0, 1])),
            "row low": (INVALID, _raw(idx, q, 5, low, [0, 1, 2, 0, 1])),
            "null scores": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], null=("scores",))),
            "null rows": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], null=("rows",))),
            "null counts": (INVALID, _raw(idx, q, 5, ok, [0, 1, 2, 0, 1], null=("counts",))),
        }
        for name, (want, res) in failing.items():
            assert res[0] == want, (name, res[0], _native.last_error())
            assert _untouched(res), f"{name}: a failing call wrote to its outputs"
        # the message names the segment and the row
        assert _raw(idx, q, 5, bad_seg3, [0, 1, 2, 0, 1])[0] == INVALID
        msg = _native.last_error()
        assert "segment 3" in msg and str(off + n) in msg, msg
        assert _raw(idx, q, 5, low, [0, 1, 2, 0, 1])[0] == INVALID and "segment 0" in _native.last_error()
        # the Python binding raises the exceptions of search_within
        with pytest.raises(ValueError):
            idx.search_segments(q, 5, bad_seg3, [0, 1, 2, 0, 1])
        with pytest.raises(ValueError):
            idx.search_segments(q, 5, ok)                      # five lists, three queries, no seg_query
        with pytest.raises(ValueError):
            idx.search_segments(q, 5, ok, [0, 1])
        with pytest.raises(ValueError):
            idx.search_segments(q[:, :d - 1], 5, ok, [0, 1, 2, 0, 1])
        # nothing to do: OK, counts 0, nothing launched
        res = _raw(idx, q, 5, [], [])
        assert res[0] == 0 and _untouched(res) and _native.last_launches() == []
        res = _raw(idx, q, 0, ok, [0, 1, 2, 0, 1])
        assert res[0] == 0 and res[3].tolist() == [0] * 5 and (res[1] == S_FILL).all() and _native.last_launches() == []
        res = _raw(idx, q, 5, [[], [], []])
        assert res[0] == 0 and res[3].tolist() == [0] * 3 and _native.last_launches() == []
        assert idx.search_segments(q, 5, [], []) == []
        assert [len(r) for _, r in idx.search_segments(q, 0, ok, [0, 1, 2, 0, 1])] == [0] * 5
        # a working call on the same handle afterwards
        got = idx.search_segments(q, 5, ok, [0, 1, 2, 0, 1])
        assert [len(r) for _, r in got] == [5, 5, 2, 4, 1]
    finally:
        idx.release()


def test_rows_longer_than_16_kib_are_unsupported(gpu):
    from svs_amd import DeviceIndex, _native
    rng = np.random.default_rng(46)
    idx = DeviceIndex(_unit(rng, 16, 4100))
    q = _unit(rng, 1, 4100)
    try:
        with pytest.raises(NotImplementedError):
            idx.search_within(q[0], 3, [1, 2, 3])
        res = _raw(idx, q, 3, [[1, 2, 3], [4]], [0, 0])
        assert res[0] == _native.SVS_ERR_UNSUPPORTED and _untouched(res)
        with pytest.raises(NotImplementedError):
            idx.search_segments(q, 3, [[1, 2, 3], [4]], [0, 0])
    finally:
        idx.release()


# ---- f. re-entrancy -----------------------------------------------------------------------------------------------------
def test_four_threads_on_one_handle(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(47)
    n, d = 9_000, 768
    idx = DeviceIndex(_unit(rng, n, d))
    qs = _unit(rng, 4, d)
    jobs = []
    for t in range(4):
        sizes = [(10, 300, 0, 4097, 64), (1, 1, 1, 900), (2000, 257), (5, 4096, 33, 0, 700, 12)][t]
        lists = [rng.choice(n, s, replace=False) for s in sizes]
        sq = [int(x) for x in rng.integers(0, 4, len(sizes))]
        jobs.append((lists, sq, idx.search_segments(qs, 20 + t, lists, sq)))
    errors = []

    def worker(t):
        lists, sq, solo = jobs[t]
        try:
            for _ in range(20):
                got = idx.search_segments(qs, 20 + t, lists, sq)
                for s in range(len(lists)):
                    if not (np.array_equal(got[s][1], solo[s][1]) and np.array_equal(got[s][0].view(np.uint32), solo[s][0].view(np.uint32))):
                        errors.append((t, s))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    try:
        ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors[:5]
        for lists, sq, solo in jobs:
            for s, rows in enumerate(lists):
                _assert_equal(solo[s], _reference(idx, qs[sq[s]], len(solo[s][1]) or 1, rows), "solo")
    finally:
        idx.release()

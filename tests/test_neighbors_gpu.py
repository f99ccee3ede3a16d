"""GPU: svs_index_neighbors (DeviceIndex.neighbors) -- the neighbours of STORED rows.

Every case is checked three ways:

  * the exact definition of include/svs_amd.h: per block of 1024 positions, ``search_batch`` of the block's stored rows at
    count + 1 with the source row removed from each list (or the last entry dropped when it is absent) -- rows and score
    BITS must be equal;
  * the oracle on the stored matrix without the source row (assert_topk_parity with f64 truth), at the tolerance the
    existing tests hold the block's route to (tests/test_batch_kernels_gpu.py: TOL, TOL_FP8_GEMV);
  * svs_internal_last_launches: rows_as_queries_kernel and drop_self_kernel ran, and the main pass is the kernel
    tests/batch_kernel_table.py names for the block's shape."""
import ctypes
import threading

import numpy as np
import pytest

from batch_kernel_table import CASES, FUSED, NF1, NF2, _tiled
from compare import assert_topk_parity
from oracle import svs_oracle as oracle
from synth import corpus_and_query
from test_batch_kernels_gpu import TOL, TOL_FP8_GEMV

pytestmark = pytest.mark.gpu

BLOCK = 1024   # SVS_NEIGHBORS_BLOCK
MINE = ("rows_as_queries_kernel", "drop_self_kernel")


def _tol(dtype, nq):
    """The bound of the route a block of nq rows takes: the single-query kernels (f32 FMAs) or a batched kernel."""
    return TOL_FP8_GEMV if dtype == "fp8" and nq == 1 else TOL[dtype]


def _bucket(nq):
    return sum(nq > b for b in (16, 32, 64, 128, 256))


def _table_kernel(dtype, d, nq, fused):
    """The main-pass kernel batch_kernel_table names for a batch of nq queries on an index of this dtype and d: the
    dispatch depends on the row length and on which query-tile bucket nq falls in, not on n."""
    bucket = (lambda q: _bucket(q)) if fused else (lambda q: min(_bucket(q), 4))   # (only the fused phased kernel changes past 256 queries)
    hits = {c[6] for c in CASES if c[0] == dtype and c[1] == d and (c[5] == FUSED) == fused and c[3] >= 2 and bucket(c[3]) == bucket(nq)}
    assert len(hits) == 1, f"batch_kernel_table has {sorted(hits)} for {dtype} d={d} nq={nq} fused={fused}"
    return hits.pop()


def _launches(n, nq, kernel=None, fused=False):
    """The calling thread's last neighbors call: both new kernels ran (the panel kernel first, over the block), and the
    main pass -- the first launch over all n rows -- is `kernel`."""
    from svs_amd import _native
    rec = _native.last_launches()
    assert rec and rec[0] == ("rows_as_queries_kernel", nq, nq), rec
    assert any(r[0] == "drop_self_kernel" for r in rec), rec
    score = [r for r in rec if r[0] not in MINE]
    main = [r for r in score if r[1] == n]
    assert main, rec
    if kernel is not None:
        assert main[0][0] == kernel, f"main pass ran {main[0][0]}, expected {kernel}: {rec}"
    if fused:
        assert score[0][1] < n, f"a fused block starts with its threshold pass over a sample: {rec}"
    elif nq > 1:
        assert all(r[1] == n for r in score), f"a materialised block has no threshold pass: {rec}"
    return rec


def _redone():
    from svs_amd import _native
    phases = (ctypes.c_double * 6)()
    assert _native.load().svs_internal_host_phases(phases, 6) == 0
    return int(phases[5])


def _definition(idx, stored, R, k):
    """The exact definition, built from search_batch; `stored` = idx.stored_rows()."""
    R = np.asarray(R, dtype=np.int64).reshape(-1)
    idx._refresh()
    count = min(max(k, 0), max(idx.n - idx.n_masked - 1, 0))
    out_s, out_r = np.empty((len(R), count), np.float32), np.empty((len(R), count), np.int64)
    for b0 in range(0, len(R), BLOCK):
        blk = R[b0:b0 + BLOCK]
        s, r = idx.search_batch(stored[blk - idx.row_offset], count + 1)
        assert s.shape == (len(blk), count + 1)
        for i, src in enumerate(blk):
            keep = np.flatnonzero(r[i] != src)[:count]      # self removed, or (absent) the last entry dropped
            assert len(keep) == count
            out_s[b0 + i], out_r[b0 + i] = s[i][keep], r[i][keep]
    return out_s, out_r


def _oracle(idx, stored, R, got_s, got_r, tol, label, dead=None, positions=None):
    """Oracle parity on the stored rows: cpu_search over the live stored matrix without the source row."""
    off = idx.row_offset
    live = np.ones(len(stored), dtype=bool) if dead is None else ~dead
    for i in (range(len(R)) if positions is None else positions):
        src = int(R[i]) - off
        others = np.flatnonzero(live & (np.arange(len(stored)) != src))
        sub, q = stored[others], stored[src]
        exp = oracle.cpu_search(sub, q, got_s.shape[1])
        truth = sub.astype(np.float64) @ q.astype(np.float64)
        pos = np.searchsorted(others, got_r[i] - off)
        assert np.all(pos < len(others)) and np.array_equal(others[np.minimum(pos, len(others) - 1)], got_r[i] - off), \
            f"{label} position {i}: a row that is masked, out of range or the source row itself"
        assert_topk_parity(got_s[i], pos, [s for s, _ in exp], [p for _, p in exp], truth64=truth,
                           label=f"{label} position {i}", score_atol=tol)
        assert np.max(np.abs(got_s[i].astype(np.float64) - truth[pos]), initial=0.0) <= tol, f"{label} position {i}"


def _check(idx, stored, R, k, label, kernel=None, fused=False, dead=None, positions=None, launches=True):
    """One neighbors call, the three checks.  Returns (scores, rows, positions re-run, the call's launch record)."""
    from svs_amd import _native
    R = np.asarray(R, dtype=np.int64).reshape(-1)
    s, r = idx.neighbors(R, k)
    rec = _native.last_launches()
    if launches and len(R) and s.shape[1]:
        _launches(idx.n, min(len(R), BLOCK), kernel, fused)
    redone = _redone() if len(R) and s.shape[1] else 0
    es, er = _definition(idx, stored, R, k)
    assert s.shape == es.shape and r.shape == er.shape, (label, s.shape, es.shape)
    assert np.array_equal(r, er), f"{label}: rows differ from the definition at {np.argwhere(r != er)[:5].tolist()}"
    assert np.array_equal(s.view(np.uint32), es.view(np.uint32)), f"{label}: score bits differ from the definition"
    assert not (r == R[:, None]).any(), f"{label}: a source row among its own neighbours"
    _oracle(idx, stored, R, s, r, _tol(idx.dtype, min(len(R), BLOCK)), label, dead, positions)
    return s, r, redone, rec


def _unit(rng, n, d):
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


# ---- single query ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_single_row_padded_gemv(gpu, dtype):
    from svs_amd import DeviceIndex
    m = _unit(np.random.default_rng(100), 1000, 100)      # ld 100 / 104 / 112: no batched kernel, the gemv loop
    idx = DeviceIndex(m, dtype=dtype)
    stored = idx.stored_rows()
    for src in (0, 517, 999):
        _check(idx, stored, [src], 10, f"{dtype} d=100 row {src}", kernel="gemv")
    idx.release()


def test_single_row_screened_f32(gpu):
    from svs_amd import DeviceIndex
    m = _unit(np.random.default_rng(1536), 40_000, 1536)   # above screen_min_rows: the screened route
    idx = DeviceIndex(m)
    assert idx.screen_stats()["shadow"] == 1
    before = idx.screen_stats()
    s, r = idx.neighbors([12_345], 10)
    rec = _launches(idx.n, 1)
    after = idx.screen_stats()
    assert after["screened"] + after["fallback"] - before["screened"] - before["fallback"] == 1, (before, after)
    assert any(x[0].startswith("gemv_f16_oneshot_kernel") for x in rec) and any(x[0].startswith("rescore_f32_kernel") for x in rec), rec
    es, er = _definition(idx, m, [12_345], 10)
    assert np.array_equal(r, er) and np.array_equal(s.view(np.uint32), es.view(np.uint32))
    _oracle(idx, m, [12_345], s, r, TOL["f32"], "screened f32")
    idx.release()


# ---- q16 / tiled / phased, materialised -----------------------------------------------------------------------------
MAT_CASES = [
    ("f32", 128, 3000, 16, None), ("f32", 128, 3001, 17, None),
    ("f16", 256, 3000, 16, None), ("f16", 256, 4097, 17, None),
    ("fp8", 256, 3000, 16, None), ("fp8", 256, 4097, 17, _tiled(32, False, 1, 128)),   # (no 17-32 query row at fp8 d = 256 in the table)
    ("f16", 512, 3000, 65, None), ("fp8", 768, 3001, 65, None),
]


@pytest.mark.parametrize("dtype,d,n,nq,kernel", MAT_CASES, ids=[f"{c[0]}-d{c[1]}-n{c[2]}-r{c[3]}" for c in MAT_CASES])
def test_materialised_blocks(gpu, dtype, d, n, nq, kernel):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(d + n + nq)
    m = _unit(rng, n, d)
    idx = DeviceIndex(m, dtype=dtype)
    stored = idx.stored_rows()
    R = rng.choice(n, nq, replace=False)
    R[0], R[-1] = n - 1, 0
    _check(idx, stored, R, 10, f"{dtype} d={d} n={n} rows={nq}", kernel=kernel or _table_kernel(dtype, d, nq, False))
    idx.release()


# ---- fused ------------------------------------------------------------------------------------------------------------
_FUSED_CORPORA = {}


def _fused_corpus(d, n, nsrc, per_src):
    """A Gaussian corpus, nsrc source rows spread over it and, for each, per_src planted near-neighbours
    (a * source + sqrt(1 - a^2) * noise, a in [0.5, 0.95]) in other 256-row tiles; built once per (d, n, nsrc)."""
    key = (d, n, nsrc)
    if key not in _FUSED_CORPORA:
        _FUSED_CORPORA.clear()
        m, _ = corpus_and_query("gaussian", 9000 + d + n % 1000, n, d, 1)
        rng = np.random.default_rng(d + nsrc)
        tiles = (n + 255) // 256
        R = (np.linspace(0, tiles - 1, nsrc).astype(np.int64) * 256 + rng.integers(0, 256, nsrc)).clip(0, n - 1)
        R[0], R[-1] = 0, n - 1
        assert len(set(R.tolist())) == nsrc
        taken = set(R.tolist())
        planted = {}
        for i, src in enumerate(R):
            rows = []
            while len(rows) < per_src:
                p = int(rng.integers(0, tiles)) * 256 + int(rng.integers(0, 256))
                if p < n and p not in taken and p // 256 != src // 256:
                    taken.add(p)
                    rows.append(p)
            a = rng.permutation(np.linspace(0.5, 0.95, per_src))
            v = rng.standard_normal((per_src, d))
            q = m[src].astype(np.float64)
            v -= np.outer(v @ q, q)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            m[rows] = (a[:, None] * q[None, :] + np.sqrt(1.0 - a * a)[:, None] * v).astype(np.float32)
            planted[i] = rows
        _FUSED_CORPORA[key] = (m, R, planted)
    return _FUSED_CORPORA[key]


FUSED_CASES = [
    ("f32", 128, NF1, 16, 255, True),     # count + 1 = 256: still fused
    ("f32", 128, NF1, 16, 256, False),    # 257: off the fused path, still right
    ("f16", 384, NF2, 257, 63, True),
    ("fp8", 768, NF1, 128, 63, True),
]


@pytest.mark.parametrize("dtype,d,n,nsrc,k,fused", FUSED_CASES, ids=[f"{c[0]}-d{c[1]}-r{c[3]}-k{c[4]}" for c in FUSED_CASES])
def test_fused_blocks_with_planted_neighbours(gpu, dtype, d, n, nsrc, k, fused):
    from svs_amd import DeviceIndex
    m, R, planted = _fused_corpus(d, n, nsrc, 6 if nsrc <= 16 else 3)
    idx = DeviceIndex(m, dtype=dtype)
    stored = m if dtype == "f32" else idx.stored_rows()
    kernel = _table_kernel(dtype, d, nsrc, fused)
    few = sorted({0, 1, nsrc // 2, nsrc - 1})              # (oracle parity on a few positions: the definition covers all)
    s, r, redone, _ = _check(idx, stored, R, k, f"{dtype} d={d} n={n} rows={nsrc} k={k}", kernel=kernel, fused=fused, positions=few)
    assert redone == 0, f"{redone} positions were re-run through the materialised path"
    assert s.shape == (nsrc, k)
    for i, rows in planted.items():
        missing = set(rows) - set(r[i].tolist())
        assert not missing, f"position {i} (row {R[i]}): planted neighbours {sorted(missing)} missing"
    idx.release()


# ---- block boundary -------------------------------------------------------------------------------------------------
def test_block_boundary_and_repeats(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(1025)
    n, d = 3000, 256
    m = _unit(rng, n, d)
    idx = DeviceIndex(m, dtype="f16")
    stored = idx.stored_rows()
    # 1025 = a block of 1024 and a block of one, which takes the single-query route
    R = rng.choice(n, 1025, replace=False)
    few = [0, 1023, 1024]
    rec = _check(idx, stored, R, 10, "1025 rows", kernel=_table_kernel("f16", d, 1024, False), positions=few)[3]
    assert [x for x in rec if x[0] == "rows_as_queries_kernel"] == [("rows_as_queries_kernel", 1024, 1024), ("rows_as_queries_kernel", 1, 1)], rec
    assert [x[2] for x in rec if x[0] == "drop_self_kernel"] == [1024, 1], rec
    assert ("gemv", n, 1) in rec and rec[1][0] == _table_kernel("f16", d, 1024, False), rec
    # 2049 positions, unsorted, with repeats: each position answered on its own
    R = rng.integers(0, n, 2049)
    R[5] = R[1500] = R[2048] = 77
    s, r, _, _ = _check(idx, stored, R, 7, "2049 rows", positions=[5, 1500, 2048], launches=False)
    assert np.array_equal(r[5], r[1500]) and np.array_equal(s[5].view(np.uint32), s[1500].view(np.uint32))
    assert np.array_equal(r[5], r[2048])    # (the block of one takes another kernel: rows, not bits)
    idx.release()


# ---- self not first / self absent -----------------------------------------------------------------------------------
def test_self_between_duplicates_short_and_zero_rows(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(64)
    n, d = 2000, 64
    m = _unit(rng, n, d)
    m[300] = m[1000]; m[1700] = m[1000]                     # exact duplicates below and above: self sits between them
    u = m[1200].copy()
    m[1200] = 0.01 * u                                      # a short row ...
    planted = [50, 350, 650, 950, 1250, 1450, 1650, 1850, 1950, 1999]
    m[planted] = u                                          # ... and 10 copies of its unit direction
    m[1500] = 0.0                                           # an all-zero row
    idx = DeviceIndex(m)
    R = [1000, 1200, 1500]
    s, r, _, _ = _check(idx, m, R, 5, "self not first / absent")
    assert r[0, 0] == 1700 and r[0, 1] == 300 and s[0, 0] == s[0, 1]           # both duplicates stay in, row desc
    assert set(r[1].tolist()) <= set(planted) and 1200 not in r[1]            # self (score 1e-4) is not in the top 6
    sb, rb = idx.search_batch(m[[1200]], 6)
    assert 1200 not in rb[0], "construction: the short row must not be among its own top 6 (the truncation branch)"
    assert np.all(s[2] == 0.0) and np.array_equal(r[2], np.arange(n - 1, n - 6, -1))   # every score 0: row desc, 1500 not among them
    # alone (single-query route) and in a larger block
    for src in R:
        _check(idx, m, [src], 5, f"row {src} alone")
    _check(idx, m, R + list(range(20)), 5, "23 rows")
    idx.release()


# ---- tombstones and offsets -----------------------------------------------------------------------------------------
def test_tombstones_offset_and_compaction(gpu):
    from svs_amd import DeviceIndex, _native
    rng = np.random.default_rng(30)
    n, d, off = 3000, 128, 10 ** 9
    m = _unit(rng, n, d)
    idx = DeviceIndex(m, row_offset=off)
    assert idx.row_offset == off
    src = np.array([5, 1400, 2999, 1400]) + off
    s0, r0, _, _ = _check(idx, m, src, 10, "offset, nothing masked")
    assert r0.min() >= off
    dead = np.zeros(n, dtype=bool)
    dead[rng.choice(n, int(0.3 * n), replace=False)] = True
    dead[r0[0, :5] - off] = True                            # the best neighbours of a source row among them
    dead[src - off] = False
    idx.mask_rows(np.flatnonzero(dead) + off)
    s1, r1, _, _ = _check(idx, m, src, 10, "30 % masked", dead=dead)
    assert not dead[r1 - off].any() and not np.isin(r0[0, :5], r1[0]).any()
    # a masked or out-of-range source row: ValueError, nothing launched, no output
    gone = int(np.flatnonzero(dead)[0]) + off
    for bad in ([src[0], gone], [src[0], off - 1], [off + n], [0]):
        with pytest.raises(ValueError) as e:
            idx.neighbors(bad, 3)
        assert _native.last_launches() == [], bad
        assert str(bad[-1]) in str(e.value)
    # after compaction, through the returned row map: the same neighbours in the new numbering
    old = idx.compact()
    assert idx.n == n - int(dead.sum()) and idx.n_masked == 0
    new_of = {int(o): p + off for p, o in enumerate(old)}
    s2, r2 = idx.neighbors([new_of[int(x)] for x in src], 10)
    assert np.array_equal(old[r2 - off], r1)
    assert np.max(np.abs(s2 - s1)) <= TOL["f32"]
    idx.release()


# ---- counts ---------------------------------------------------------------------------------------------------------
def test_counts(gpu):
    from svs_amd import DeviceIndex, _native
    rng = np.random.default_rng(9)
    m = _unit(rng, 50, 32)
    idx = DeviceIndex(m)
    R = [3, 49, 0]
    s, r = idx.neighbors(R, 0)
    assert s.shape == (3, 0) and r.shape == (3, 0) and _native.last_launches() == []
    s, r = idx.neighbors(R, -4)
    assert s.shape == (3, 0) and _native.last_launches() == []
    for k in (1000, 2 ** 31 - 1, 2 ** 40):                  # k > n: rank everything but the row itself
        s, r, _, _ = _check(idx, m, R, k, f"k={k}")
        assert s.shape == (3, 49)
        assert all(sorted(r[i].tolist()) == [x for x in range(50) if x != R[i]] for i in range(3))
    s, r = idx.neighbors(np.array([], dtype=np.int64), 5)
    assert s.shape == (0, 5) and r.shape == (0, 5) and _native.last_launches() == []
    # the C ABI: stride k, entries past count untouched, *out_count written
    lib = _native.load()
    rows = np.array(R, dtype=np.int64)
    out_s, out_r = np.full((3, 60), 7.0, np.float32), np.full((3, 60), -7, np.int64)
    cnt = ctypes.c_int32(-1)
    assert lib.svs_index_neighbors(idx._handle(), rows.ctypes.data, 3, 60, out_s.ctypes.data, out_r.ctypes.data, ctypes.byref(cnt)) == 0
    assert cnt.value == 49
    assert np.all(out_s[:, 49:] == 7.0) and np.all(out_r[:, 49:] == -7)
    es, er = _definition(idx, m, R, 60)
    assert np.array_equal(out_r[:, :49], er) and np.array_equal(out_s[:, :49].view(np.uint32), es.view(np.uint32))
    cnt = ctypes.c_int32(-1)
    assert lib.svs_index_neighbors(idx._handle(), rows.ctypes.data, -1, 5, out_s.ctypes.data, out_r.ctypes.data, ctypes.byref(cnt)) == _native.SVS_ERR_INVALID
    cnt = ctypes.c_int32(-1)
    assert lib.svs_index_neighbors(idx._handle(), None, 0, 5, None, None, ctypes.byref(cnt)) == 0 and cnt.value == 5
    idx.release()
    one = DeviceIndex(m[:1])                                  # n = 1: count 0
    s, r = one.neighbors([0], 5)
    assert s.shape == (1, 0) and _native.last_launches() == []
    one.release()
    two = DeviceIndex(m[:2])                                  # n = 2: the other row
    s, r, _, _ = _check(two, m[:2], [0, 1, 1], 5, "n=2")
    assert r.tolist() == [[1], [0], [0]]
    two.release()


# ---- overflow re-run ------------------------------------------------------------------------------------------------
def test_overflowed_positions_are_rerun(gpu, first_rows_thresholds):
    """Thresholds from the first rows (random), source rows from one tight cluster behind them: every cluster row passes
    every source row's threshold, the candidate lists overflow, and the positions are re-run from a panel of their own."""
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(384)
    n, d, head, k = NF1, 384, 20_000, 64
    m = np.empty((n, d), dtype=np.float32)
    m[:head] = _unit(rng, head, d)
    centre = _unit(rng, 1, d)[0]
    m[head:] = centre + 1e-3 * rng.standard_normal((n - head, d), dtype=np.float32)
    m[head:] /= np.linalg.norm(m[head:], axis=1, keepdims=True)
    R = head + rng.choice(n - head, 32, replace=False)
    # the construction, on the CPU: the (k + 1)-th best score among the threshold rows (the first max(16384, n / 64)) is far
    # below every cluster score, for every source row
    sc = m[:16_384] @ m[R].T
    thr = np.sort(sc, axis=0)[-(k + 1)]
    cluster = m[head:head + 4096] @ m[R].T
    assert thr.max() < 0.3 and cluster.min() > 0.99, (thr.max(), cluster.min())
    idx = DeviceIndex(m, dtype="f16")
    stored = idx.stored_rows()
    s, r = idx.neighbors(R, k)
    redone = _redone()
    rec = _launches(n, 32, fused=True)
    assert redone > 0, "no position overflowed: nothing was re-run"
    assert sum(x[0] == "rows_as_queries_kernel" for x in rec) == 2 and sum(x[0] == "drop_self_kernel" for x in rec) == 2, rec
    es, er = _definition(idx, stored, R, k)
    assert _redone() == redone                                 # (the definition's search_batch overflowed too)
    assert np.array_equal(r, er) and np.array_equal(s.view(np.uint32), es.view(np.uint32))
    assert r.min() >= head and not (r == R[:, None]).any()
    idx.release()


# ---- re-entrancy ----------------------------------------------------------------------------------------------------
def test_concurrent_calls_on_one_handle(gpu):
    from svs_amd import DeviceIndex
    rng = np.random.default_rng(5)
    n, d = 20_000, 256
    m = _unit(rng, n, d)
    idx = DeviceIndex(m, dtype="f16")
    sets = [np.arange(t, n, 4)[:300 + 37 * t] for t in range(4)]
    qs = _unit(rng, 40, d)
    solo = [idx.neighbors(R, 10) for R in sets]
    solo_search = idx.search_batch(qs, 10)
    out, errs = {}, []

    def nb(t):
        try:
            for _ in range(3):
                out[t] = idx.neighbors(sets[t], 10)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    def sb():
        try:
            for _ in range(6):
                out["s"] = idx.search_batch(qs, 10)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=nb, args=(t,)) for t in range(4)] + [threading.Thread(target=sb)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, errs
    for t in range(4):
        assert np.array_equal(out[t][1], solo[t][1]) and np.array_equal(out[t][0].view(np.uint32), solo[t][0].view(np.uint32)), t
    assert np.array_equal(out["s"][1], solo_search[1]) and np.array_equal(out["s"][0], solo_search[0])
    idx.release()

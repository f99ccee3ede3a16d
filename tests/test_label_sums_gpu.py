"""GPU: per-label row sums (svs_index_label_sums; svs_amd/csrc/label_sums.h) and DeviceIndex.kmeans against their
definitions.

The truth is ``label_sums_model.replay`` over ``idx.stored_rows()``: the same f64 additions in the same order, so every
comparison of sums is BIT equality.  Data: 4,099 rows (no multiple of 4, 64, 256 or the 1,024-row strip; five strips),
d = 64 and d = 100 (ragged 16-byte pieces and padding in f16 / fp8), unit-norm Gaussian rows -- on which the definition
is the exact sum, so only the WIDE cases (rows scaled by 2^-20 .. 2^20) can tell a wrong ORDER from the right one; they
assert that the reversed order gives other bits."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import assign_model as am
import label_sums_model as lm
import svs_amd
from svs_amd import _native

pytestmark = pytest.mark.gpu

N = 4099
DIMS = [64, 100]
DTYPES = ["f32", "f16", "fp8"]
SEED = 20263
RANGES = [(1, 4097), (4037, 62), (64, 64), (2050, 1), (0, N)]      # (row0, nrows); the last is the whole index
SETS = [1, 2, 65, 1024]
KERNELS = ["label_sums_hist_kernel", "label_sums_scan_kernel", "label_sums_plan_kernel", "label_sums_scatter_kernel",
           "label_sums_chunk_kernel", "label_sums_fold_kernel"]


def _names():
    return [k for k, _, _ in _native.last_launches()]


def _values(rng):
    """1,200 distinct label values, 0 and 2^32 - 1 among them, and per-row labels drawn from the first 1,100 with a skew
    (a few labels hold hundreds of rows, most a handful, some none)."""
    vals = np.unique(np.concatenate([rng.integers(0, 2 ** 32, size=1300, dtype=np.uint64), [0, 2 ** 32 - 1]]))[:1200]
    vals = rng.permutation(vals).astype(np.uint32)
    w = 1.0 / (1.0 + np.arange(1100)) ** 0.8
    w[0] = w[1:].sum() / 4.0          # one label holds a fifth of the rows: several chunks
    lab = vals[rng.choice(1100, size=N, p=w / w.sum())]
    return vals, lab


def _label_set(rng, vals, lab, nset):
    """``nset`` distinct labels, unsorted -- present ones (the most frequent first among them) and absent ones -- plus
    three repeats (a set of one: the label repeated)."""
    present = np.unique(lab)
    top = present[np.bincount(np.searchsorted(present, lab)).argmax()]
    others = rng.permutation(np.setdiff1d(present, [top]))
    absent = rng.permutation(np.setdiff1d(vals, present))
    n_pre = min(len(others), nset - 1 - nset // 4)
    pick = np.concatenate([[top], others[:n_pre], absent[:nset - 1 - n_pre]])
    assert len(np.unique(pick)) == nset
    pick = rng.permutation(pick)
    return np.concatenate([pick, pick[rng.integers(0, nset, size=3)]]).astype(np.uint32)


@pytest.fixture(scope="module", params=[(d, dt) for d in DIMS for dt in DTYPES], ids=lambda p: f"d{p[0]}-{p[1]}")
def case(request, gpu):
    d, dtype = request.param
    rng = np.random.default_rng(SEED + d)
    m = lm.unit(rng, N, d)
    vals, lab = _values(rng)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    idx.set_labels(lab)
    stored = idx.stored_rows()
    for a in (m, stored, vals, lab):
        a.setflags(write=False)
    yield SimpleNamespace(idx=idx, m=m, stored=stored, vals=vals, lab=lab, d=d, dtype=dtype)
    idx.release()


@pytest.mark.parametrize("nset", SETS)
def test_bit_equality_with_the_replay(case, nset):
    k = case
    labels = _label_set(np.random.default_rng(nset), k.vals, k.lab, nset)
    for row0, nrows in RANGES:
        sl = slice(row0, row0 + nrows)
        want, wcounts = lm.replay(k.stored[sl], k.lab[sl], None, labels)
        col = k.idx.label_sums(labels, row0=row0, nrows=nrows)                              # the column
        assert _names() == KERNELS
        arg = k.idx.label_sums(labels, row_labels=k.lab[sl], row0=row0, nrows=nrows)      # the caller's labels
        for s, c in (col, arg):
            assert s.dtype == np.float64 and s.shape == (len(labels), k.d) and c.dtype == np.int64
            assert np.array_equal(c, wcounts), (row0, nrows)
            assert lm.same_bits(s, want), (row0, nrows, int((s != want).sum()))
        if nrows == N:      # a label of several chunks is in every set, labels absent from the data in the larger ones
            assert wcounts.max() > 513 and (wcounts == 0).any() == (nset >= 65)
    # the default range is the whole index; means divide in f64 and cast
    s, c = k.idx.label_sums(labels)
    assert lm.same_bits(s, want) and np.array_equal(c, wcounts)
    mean, c2 = k.idx.label_means(labels)
    assert mean.dtype == np.float32 and np.array_equal(c2, wcounts)
    assert np.array_equal(mean, lm.means(want, wcounts).astype(np.float32)) and not mean[wcounts == 0].any()


@pytest.mark.parametrize("d", DIMS)
def test_f16_sums_are_exact(gpu, d):
    """Halves have 11 significant bits in a narrow exponent range: every partial sum is representable, the chunked sum IS
    the sum."""
    rng = np.random.default_rng(SEED + d)
    m = lm.unit(rng, N, d)
    vals, lab = _values(rng)
    labels = _label_set(np.random.default_rng(9), vals, lab, 65)
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    try:
        s, c = idx.label_sums(labels, row_labels=lab)
        want, wcounts = lm.exact(idx.stored_rows(), lab, None, labels)
        assert np.array_equal(c, wcounts) and c.max() > 256 and lm.same_bits(s, want)
    finally:
        idx.release()


def test_planted_label_sizes_at_the_chunk_edges(case):
    k = case
    sizes = {11: 0, 12: 1, 13: 255, 14: 256, 15: 257, 16: 512, 17: 513}
    rl = np.full(N, 99, dtype=np.uint32)
    rows = np.random.default_rng(1).permutation(N)
    at = 0
    for label, size in sizes.items():
        rl[rows[at:at + size]] = label
        at += size
    labels = list(sizes) + [99]
    s, c = k.idx.label_sums(labels, row_labels=rl)
    want, wcounts = lm.replay(k.stored, rl, None, labels)
    assert c.tolist() == list(sizes.values()) + [N - at] and np.array_equal(c, wcounts)
    assert lm.same_bits(s, want)
    assert not s[0].any() and not np.signbit(s[0]).any()          # the empty label: +0.0 everywhere


def test_tombstones_and_compaction(case):
    k = case
    idx = svs_amd.DeviceIndex(k.m, dtype=k.dtype)
    try:
        idx.set_labels(k.lab)
        present, cnt = np.unique(k.lab, return_counts=True)
        big = present[cnt.argmax()]
        mine = np.flatnonzero(k.lab == big)
        assert len(mine) >= 515
        # inside and at the edges of the big label's chunks, and rows of other labels, the first and the last row among them
        dead = sorted(set(mine[[0, 1, 255, 256, 257, 300, 511, 512, len(mine) - 1]].tolist()) | {0, 5, 1023, 1024, 2047, N - 1})
        labels = [big] + [l for l in present[:40] if l != big] + [int(k.lab[0]), int(k.lab[N - 1])]
        idx.mask_rows(dead)
        live = np.ones(N, dtype=bool)
        live[dead] = False
        want, wcounts = lm.replay(k.stored, k.lab, live, labels)
        s, c = idx.label_sums(labels)
        assert np.array_equal(c, wcounts) and c[0] == len(mine) - len(set(dead) & set(mine.tolist()))
        assert lm.same_bits(s, want)                       # exactly those rows left, and the chunks moved up behind them
        s2, c2 = idx.label_sums(labels, row_labels=k.lab)
        assert lm.same_bits(s2, want) and np.array_equal(c2, wcounts)
        old = idx.compact()
        assert np.array_equal(old, np.flatnonzero(live)) and idx.n == N - len(dead)
        s3, c3 = idx.label_sums(labels)                    # the column was carried along; the live rows' order is the same
        assert lm.same_bits(s3, want) and np.array_equal(c3, wcounts)
        s4, c4 = idx.label_sums(labels, row_labels=k.lab[live])
        assert lm.same_bits(s4, want) and np.array_equal(c4, wcounts)
    finally:
        idx.release()


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", ["f32", "fp8"])
def test_wide_data_pins_the_order(gpu, d, dtype):
    """The test that fails if rows are added in another order: rows scaled by 2^-20 .. 2^20, one label with more than
    2,000 rows (eight chunks and more)."""
    rng = np.random.default_rng(SEED + d)
    m = lm.wide(rng, N, d)
    rl = np.where(rng.random(N) < 0.55, 7, rng.integers(0, 3, size=N)).astype(np.uint32)
    assert (rl == 7).sum() > 2000
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        stored = idx.stored_rows()
        labels = [2, 7, 0, 1]
        s, c = idx.label_sums(labels, row_labels=rl)
        want, wcounts = lm.replay(stored, rl, None, labels)
        assert np.array_equal(c, wcounts) and lm.same_bits(s, want)
        for name, kw in (("reversed", dict(order=lambda r: r[::-1])), ("chunk 128", dict(chunk=128)), ("one chain", dict(chunk=None))):
            other, _ = lm.replay(stored, rl, None, labels, **kw)
            differ = int((other.view(np.uint64) != want.view(np.uint64)).sum())
            print(f"{dtype} d={d} {name}: {differ} of {want.size} elements differ from the definition's order")
            assert differ >= 1 and not lm.same_bits(s, other), name
        idx.set_labels(rl)
        s2, c2 = idx.label_sums(labels)
        assert lm.same_bits(s2, want) and np.array_equal(c2, wcounts)
        # bit-reproducible, and independent of the other labels of the set
        s3, _ = idx.label_sums([7])
        assert lm.same_bits(s3[0], want[1])
    finally:
        idx.release()


def test_rows_of_16_kib_and_wider(gpu):
    rng = np.random.default_rng(4)
    m = lm.unit(rng, 300, 4096)
    rl = rng.integers(0, 3, size=300).astype(np.uint32)
    idx = svs_amd.DeviceIndex(m)
    try:
        s, c = idx.label_sums([1, 0, 2, 5], row_labels=rl)
        want, wcounts = lm.replay(idx.stored_rows(), rl, None, [1, 0, 2, 5])
        assert np.array_equal(c, wcounts) and lm.same_bits(s, want) and c.sum() == 300
    finally:
        idx.release()
    idx = svs_amd.DeviceIndex(lm.unit(rng, 40, 4097))
    try:
        with pytest.raises(NotImplementedError, match="16 KiB"):
            idx.label_sums([0])
        s, c = idx.label_sums([0], sums=False)          # no row is read for the counts
        assert s is None and c.tolist() == [40]
    finally:
        idx.release()


def test_count_only_call_runs_the_histogram_alone(case):
    k = case
    labels = _label_set(np.random.default_rng(2), k.vals, k.lab, 65)
    s, c = k.idx.label_sums(labels, sums=False)
    assert _names() == KERNELS[:2]
    assert s is None and np.array_equal(c, lm.replay(k.stored, k.lab, None, labels)[1])
    k.idx.label_sums(labels)
    assert _names() == KERNELS


def test_c_entry_errors_write_nothing(case):
    k = case
    lib, h = _native.load(), k.idx._handle()
    labels = np.array([3, 1, 2], dtype=np.uint32)
    sums = np.full((3, k.d), -7.0)
    counts = np.full(3, -7, dtype=np.int64)

    def call(lab=labels, nlabels=3, row0=0, nrows=N, rl=None, out=sums, cnt=counts, handle=h):
        return lib.svs_index_label_sums(handle, None if lab is None else lab.ctypes.data, nlabels, row0, nrows,
                                        None if rl is None else rl.ctypes.data, None if out is None else out.ctypes.data,
                                        None if cnt is None else cnt.ctypes.data)

    many = np.arange(1025, dtype=np.uint32)
    big_s, big_c = np.full((1025, k.d), -7.0), np.full(1025, -7, dtype=np.int64)
    for rc, kw in ((_native.SVS_ERR_INVALID, dict(nlabels=-1)), (_native.SVS_ERR_INVALID, dict(nrows=-1)),
                   (_native.SVS_ERR_INVALID, dict(lab=None)), (_native.SVS_ERR_INVALID, dict(row0=1)),
                   (_native.SVS_ERR_INVALID, dict(row0=-1, nrows=5)), (_native.SVS_ERR_INVALID, dict(row0=N + 1, nrows=0)),
                   (_native.SVS_ERR_INVALID, dict(handle=None)),
                   (_native.SVS_ERR_UNSUPPORTED, dict(lab=many, nlabels=1025, out=big_s, cnt=big_c))):
        assert call(**kw) == rc, kw
        assert _names() == []
    assert (sums == -7.0).all() and (counts == -7).all() and (big_s == -7.0).all() and (big_c == -7).all()
    # 1,024 distinct labels with repeats on top are fine
    ok = np.concatenate([many[:1024], many[:5]])
    ok_s, ok_c = np.full((1029, k.d), -7.0), np.full(1029, -7, dtype=np.int64)
    assert call(lab=ok, nlabels=1029, out=ok_s, cnt=ok_c) == _native.SVS_OK and ok_c.sum() >= 0 and (ok_c[:5] == ok_c[1024:]).all()
    # nothing to do: SVS_OK, nothing launched, nothing written ...
    assert call(nlabels=0) == _native.SVS_OK and call(out=None, cnt=None) == _native.SVS_OK and _names() == []
    assert (sums == -7.0).all() and (counts == -7).all()
    # ... and an empty range zeroes what it is given
    assert call(row0=17, nrows=0) == _native.SVS_OK and _names() == []
    assert not sums.any() and not np.signbit(sums).any() and not counts.any()
    # an empty index
    e = svs_amd.DeviceIndex(np.zeros((0, k.d), dtype=np.float32))
    try:
        sums[:] = -7.0
        assert call(handle=e._handle(), nrows=0) == _native.SVS_ERR_SHAPE and (sums == -7.0).all()
    finally:
        e.release()


def test_fresh_index_allocates_no_column(gpu):
    rng = np.random.default_rng(6)
    m = lm.unit(rng, 1500, 64)
    idx = svs_amd.DeviceIndex(m, dtype="f16")
    try:
        before = idx.hbm_bytes
        s, c = idx.label_sums([5, 0])                      # no column: every row carries label 0
        idx._refresh()
        assert idx.hbm_bytes == before
        stored = idx.stored_rows()
        want, wcounts = lm.replay(stored, np.zeros(1500, dtype=np.uint32), None, [5, 0])
        assert c.tolist() == [0, 1500] and lm.same_bits(s, want)
        rl = rng.integers(0, 4, size=1500).astype(np.uint32)
        s, c = idx.label_sums([3, 3, 1], row_labels=rl)
        idx._refresh()
        assert idx.hbm_bytes == before and lm.same_bits(s, lm.replay(stored, rl, None, [3, 3, 1])[0])
        assert idx.labels().tolist() == [0] * 1500
        with pytest.raises(ValueError, match="row labels"):
            idx.label_sums([1], row_labels=rl[:-1])
    finally:
        idx.release()


def _model_centroids(stored, best, live, previous):
    """The update step over the model's sums: the normalised f64 means of the final assignment, cast to f32."""
    s, c = lm.replay(stored, best.astype(np.uint32), live, np.arange(len(previous), dtype=np.uint32))
    mean = lm.means(s, c)
    norm = np.sqrt((mean * mean).sum(axis=1))
    out = previous.copy()
    has = c > 0
    out[has] = (mean[has] / norm[has, None]).astype(np.float32)
    return out, c


@pytest.mark.parametrize("dtype", DTYPES)
def test_kmeans_recovers_planted_clusters(gpu, dtype):
    rng = np.random.default_rng(SEED)
    n, d, c = 1500, 64, 5
    planted = rng.integers(0, c, size=n)
    x = np.eye(d)[planted] + 0.02 * rng.standard_normal((n, d))
    m = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    idx = svs_amd.DeviceIndex(m, dtype=dtype)
    try:
        stored = idx.stored_rows()
        first = np.array([np.flatnonzero(planted == j)[0] for j in range(c)])
        far = -np.ones((1, d), dtype=np.float32) / np.float32(np.sqrt(d))          # no row's nearest: an empty cluster
        init = np.concatenate([m[first], far])
        cent, best, scores, counts, ran = idx.kmeans(c + 1, init=init)
        assert cent.dtype == np.float32 and cent.shape == (c + 1, d) and best.dtype == np.int32 and counts.dtype == np.int64
        assert 1 <= ran <= 10
        # every row's margin between its best and second-best centroid exceeds the tolerance of an f32 assignment, on
        # the stored values of both sides: the partition is then determined
        tmp = svs_amd.DeviceIndex(cent, dtype=dtype)
        try:
            vstored = tmp.stored_rows()
        finally:
            tmp.release()
        _, tol = am.tolerances(stored, vstored, d)
        assert am.margins(stored, vstored).min() > tol
        # the planted partition, up to relabelling (here: none, the initial centroids fix the names)
        assert np.array_equal(best, planted) and np.array_equal(counts, np.bincount(planted, minlength=c + 1))
        assert counts[c] == 0 and np.array_equal(cent[c].view(np.uint32), init[c].view(np.uint32))     # kept its initial centroid
        want, wc = _model_centroids(stored, best, None, init)
        assert np.array_equal(wc, counts) and np.array_equal(cent.view(np.uint32), want.view(np.uint32))
        # seeded runs: identical in every bit, and a partition of the same quality
        a = idx.kmeans(c, iterations=6, seed=11)
        b = idx.kmeans(c, iterations=6, seed=11)
        for u, v in zip(a[:4], b[:4]):
            assert np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
        assert a[4] == b[4] and a[3].sum() == n
        wa, _ = _model_centroids(stored, a[1], None, np.zeros((c, d), dtype=np.float32))
        assert np.array_equal(a[0][a[3] > 0].view(np.uint32), wa[a[3] > 0].view(np.uint32))
        # write_labels: the column holds the clusters, and a labelled search per cluster returns only its rows
        before = idx.hbm_bytes
        cent2, best2, _, counts2, _ = idx.kmeans(c + 1, init=init, write_labels=True)
        assert np.array_equal(best2, planted) and idx.hbm_bytes > before
        assert np.array_equal(idx.labels(), planted.astype(np.uint32))
        for j in range(c):
            hits, matched = idx.search_labeled(cent2[j], 40, [j])
            assert matched == counts2[j] and len(hits) == 40 and all(best2[r] == j for _, r in hits)
        # tombstoned rows have no weight
        dead = np.flatnonzero(planted == 0)[:7]
        idx.mask_rows(dead)
        live = np.ones(n, dtype=bool)
        live[dead] = False
        cent3, best3, _, counts3, _ = idx.kmeans(c + 1, init=init)
        want3, wc3 = _model_centroids(stored, best3, live, init)
        assert np.array_equal(counts3, wc3) and counts3[0] == counts[0] - 7 and np.array_equal(cent3.view(np.uint32), want3.view(np.uint32))
        with pytest.raises(ValueError):
            idx.kmeans(1025)
    finally:
        idx.release()


def test_timing_hook(case):
    k = case
    lib = _native.load()
    ms = C.c_double(0.0)
    _native.check(lib.svs_index_set_timing(k.idx._handle(), 1))
    try:
        k.idx.label_sums([int(k.lab[0])])
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(ms)))
        assert ms.value > 0.0
        k.idx.label_sums([int(k.lab[0])], sums=False)
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(ms)))
        assert ms.value == -1.0
        # a call that fails validation leaves no earlier call's time behind
        k.idx.label_sums([int(k.lab[0])])
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(ms)))
        assert ms.value > 0.0
        assert lib.svs_index_label_sums(k.idx._handle(), None, -1, 0, N, None, None, None) == _native.SVS_ERR_INVALID
        _native.check(lib.svs_internal_label_sums_kernel_ms(C.byref(ms)))
        assert ms.value == -1.0
    finally:
        _native.check(lib.svs_index_set_timing(k.idx._handle(), 0))

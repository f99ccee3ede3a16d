"""GPU: svs_index_search_device with more than one query -- the entry ShardedIndex.search_batch hands a whole batch to,
and what svs_index_search_device_ahead becomes whenever nq != 1 -- against exact references.

The batched device entry is not the host entry with other pointers: it is never fused, it hands k and count to the
selection kernels separately (they write the -inf / -1 padding at stride k themselves), it stages the queries from the
caller's pointer (aliased, copied or converted, depending on shape and alignment), and it returns without synchronising
on a context it picks by stream.  Groups:

  A. every materialised batched route of tests/batch_kernel_table.py through the device entry: the kernel is asserted
     by name, the whole (nq, n) score matrix is compared with f64 under the bounds of test_batch_kernels_gpu.py, and the
     records equal the host entry's bit for bit;
  B. the delivery contract: stride k, padding past count (k > n; tombstones with live < k <= n) on the FINAL, WINDOW
     and SORT selection paths, row_offset, k <= 0, a wrong d;
  C. query pointer forms: a base one float past a 16-byte boundary, d = 100 (per-query loop), ld != d (copy path);
  D. stream semantics with one synchronisation at the end: scratch growth under pending work, two streams on one
     handle, producer and consumer ordering, svs_index_search_device_ahead with nq = 5 behind a ready event;
  E. never fused: 131,329 rows x 16 queries run materialised and equal the host entry's fused answer;
  F. ShardedIndex.search_batch at one rank (the Python consumer of the record layout).

Every output starts as NaN / -7 between guards of the same; every query buffer is a view into NaN (device_entry.py).
Each test prints the largest |score - f64| it saw next to the bound it is held to.
"""
import numpy as np
import pytest

from batch_kernel_table import CASES, MAT, NF1, NORMS, _q16, _tiled, case_id
from compare import SCORE_ATOL
from device_entry import Outputs, QueryBuf, bits, check_topk, same_bits, search_device
from synth import corpus_and_query
from test_batch_kernels_gpu import TOL, TOL_FP8_GEMV, _f64_scores, _main_pass, _stored_queries

pytestmark = pytest.mark.gpu

ROW_OFFSET = 10 ** 12


@pytest.fixture(scope="module")
def dev(gpu):
    """(torch, cuda:0, a stream of the module's own)"""
    import torch
    d = torch.device("cuda:0")
    return torch, d, torch.cuda.Stream(device=d)


def _one_call(dev, idx, q, k, offset=0):
    """All of q through one device call on the module's stream, then ONE synchronise.
    -> (scores (nq, k), rows (nq, k), count, launches recorded at the call)"""
    from svs_amd import _native
    torch, d, st = dev
    qb = QueryBuf(torch, d, q, offset)
    out = Outputs(torch, d, q.shape[0], k)
    torch.cuda.synchronize(d)
    count = search_device(idx, qb, k, out, st)
    launches = _native.last_launches()
    st.synchronize()
    s, r = out.host()
    return s, r, count, launches


def _main_kernel(launches, n, kernel):
    """The table's kernel ran over all n rows, and nothing ran over fewer (no threshold pass: not fused)."""
    assert launches and all(rec[1] == n for rec in launches), f"a launch over fewer than {n} rows: {launches}"
    assert launches[0][0] == kernel, f"main pass ran {launches[0][0]}, expected {kernel} ({launches})"


def _stored(idx, m, qs, dtype):
    return (m if dtype == "f32" else idx.stored_rows()), _stored_queries(qs, dtype)


# ---- A. every materialised batched route, the whole score matrix ---------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[5] in (MAT, NORMS)], ids=case_id)
def test_materialised_route_through_device_entry(dev, case):
    from svs_amd import DeviceIndex
    torch, tdev, st = dev
    dtype, d, n, nq, k, form, kernel = case
    assert k == n
    m, qs = corpus_and_query("gaussian", 5000 + d + nq + n % 997, n, d, nq)   # (the corpus of test_batch_kernels_gpu.py)
    if form == NORMS:
        rng = np.random.default_rng(d + nq)
        m *= (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)[:, None]
        qs *= (10.0 ** rng.uniform(-1, 1, nq)).astype(np.float32)[:, None]
    idx = DeviceIndex(m, dtype=dtype)
    qb = QueryBuf(torch, tdev, qs)
    out = Outputs(torch, tdev, nq, k)
    torch.cuda.synchronize(tdev)
    count = search_device(idx, qb, k, out, st)
    _main_pass(n, nq, kernel, fused=False)
    st.synchronize()
    s, r = out.host()
    hs, hr = idx.search_batch(qs, n)
    md = m if dtype == "f32" else idx.stored_rows()
    idx.release()
    assert count == n
    assert not np.isnan(s).any(), "NaN scores: a read outside the queries, or an entry nobody wrote"
    assert np.array_equal(np.sort(r, axis=1), np.broadcast_to(np.arange(n), (nq, n))), "row lists are not permutations"
    ds = np.diff(s, axis=1)
    assert np.all(ds <= 0) and np.all(np.diff(r, axis=1)[ds == 0] < 0), "not in (score desc, row desc) order"
    got = np.empty((nq, n))
    np.put_along_axis(got, r, s.astype(np.float64), axis=1)
    qd = _stored_queries(qs, dtype)
    err = np.abs(got - _f64_scores(md, qd).T)
    tol = TOL_FP8_GEMV if dtype == "fp8" and kernel == "gemv" else TOL[dtype]
    if form == NORMS:
        err = err / (np.linalg.norm(qd.astype(np.float64), axis=1)[:, None] * np.linalg.norm(md.astype(np.float64), axis=1)[None, :])
    q, row = np.unravel_index(np.argmax(err), err.shape)
    print(f"DEVBATCH A {dtype} {kernel} d={d} n={n} nq={nq} {form}: max err {err[q, row]:.3g} (bound {tol})")
    assert err[q, row] <= tol, f"{kernel} {dtype} d={d} n={n} nq={nq} {form}: max |score - f64| = {err[q, row]:.3g} at query {q}, row {row}"
    # the host entry on the same handle: same kernels, same operands -> the same records, bit for bit
    same_bits((s, r), (hs, hr), f"{kernel} {dtype} d={d} nq={nq}: device entry vs host entry")


# ---- B. delivery contract ----------------------------------------------------------------------------------------------
B_D = {"f32": 128, "f16": 256, "fp8": 128}
B_CASES = (
    # (label, dtype, n, masked rows, nq, k): count = min(k, n - masked)
    # k > n, FINAL path (n <= 4096): every dtype's score routes at 2, 3 and 17 queries
    [(f"final-k>n-{dt}-q{nq}", dt, 40, 0, nq, 101) for dt in ("f32", "f16", "fp8") for nq in (2, 3, 17)] +
    # k > n, SORT path (n > 4096, count > 2048)
    [("sort-k>n-f32-q3", "f32", 5000, 0, 3, 5001), ("sort-k>n-fp8-q17", "fp8", 5000, 0, 17, 5001)] +
    # tombstones: live < k <= n
    [(f"final-masked-{dt}-q{nq}", dt, 300, 250, nq, 101) for dt, nq in (("f32", 2), ("f16", 3), ("fp8", 17))] +
    [("window-masked-f32-q3", "f32", 6000, 4100, 3, 2000), ("window-masked-f16-q17", "f16", 6000, 4100, 17, 2000),
     ("window-masked-fp8-q2", "fp8", 6000, 4100, 2, 1999)] +
    [("sort-masked-f32-q2", "f32", 9000, 2000, 2, 8001)] +
    # no padding at all: odd k <= live rows, with and without tombstones
    [("final-k7-f16-q3", "f16", 300, 0, 3, 7), ("window-k7-masked-f32-q17", "f32", 6000, 100, 17, 7)]
)


@pytest.mark.parametrize("label,dtype,n,n_dead,nq,k", B_CASES, ids=[c[0] for c in B_CASES])
def test_delivery_stride_padding_row_offset(dev, label, dtype, n, n_dead, nq, k):
    from svs_amd import DeviceIndex
    d = B_D[dtype]
    m, qs = corpus_and_query("gaussian", 600 + n + nq + k, n, d, nq)
    idx = DeviceIndex(m, dtype=dtype, row_offset=ROW_OFFSET)
    dead = None
    if n_dead:
        rng = np.random.default_rng(n + n_dead)
        best = idx.search_batch(qs, 5)[1].reshape(-1) - ROW_OFFSET       # the winners go first: masking must change the answer
        rest = np.setdiff1d(np.arange(n), best)
        dead = np.sort(np.concatenate([np.unique(best), rng.choice(rest, n_dead - np.unique(best).size, replace=False)]))
        idx.mask_rows(dead + ROW_OFFSET)
        assert idx.n_masked == n_dead
    s, r, count, launches = _one_call(dev, idx, qs, k)
    assert all(rec[1] == n for rec in launches), launches
    md, qd = _stored(idx, m, qs, dtype)
    idx.release()
    worst = check_topk(s, r, count, md, qd, label, dead=dead, row_offset=ROW_OFFSET)
    print(f"DEVBATCH B {dtype} {label}: count {count} of k {k}, max err {worst:.3g} (bound {SCORE_ATOL})")


@pytest.mark.parametrize("k", [0, -3])
def test_k_not_positive_writes_nothing(dev, k):
    from svs_amd import DeviceIndex
    torch, tdev, st = dev
    m, qs = corpus_and_query("gaussian", 71, 300, 128, 3)
    idx = DeviceIndex(m)
    qb = QueryBuf(torch, tdev, qs)
    out = Outputs(torch, tdev, 3, 4)
    torch.cuda.synchronize(tdev)
    assert search_device(idx, qb, k, out, st) == 0
    assert idx.search_device(qb.ptr, 3, 128, k, 0, 0, st.cuda_stream) == 0          # null outputs are accepted
    assert idx.search_device_ahead(qb.ptr, 3, 128, k, 0, 0, st.cuda_stream) == 0
    st.synchronize()
    assert out.untouched()
    idx.release()


def test_wrong_d_with_many_queries_is_a_value_error(dev):
    from svs_amd import DeviceIndex
    torch, tdev, st = dev
    m, qs = corpus_and_query("gaussian", 72, 300, 128, 3)
    idx = DeviceIndex(m)
    qb = QueryBuf(torch, tdev, qs)
    out = Outputs(torch, tdev, 3, 7)
    torch.cuda.synchronize(tdev)
    for d in (127, 64, 129):
        with pytest.raises(ValueError):
            idx.search_device(qb.ptr, 2, d, 7, *out.ptrs, st.cuda_stream)
        with pytest.raises(ValueError):
            idx.search_device_ahead(qb.ptr, 2, d, 7, *out.ptrs, st.cuda_stream)
    st.synchronize()
    assert out.untouched()
    idx.release()


# ---- C. query pointer forms ----------------------------------------------------------------------------------------------
C_CASES = [
    # (label, dtype, d, nq, kernel of the main pass)
    # 1. a q16 shape (fp8 has no 16-query kernel: its 16 queries take the tiled one).  f32: ld == d and 16 queries would alias
    ("q16-f32", "f32", 128, 16, _q16("f32", False)),
    ("q16-f16", "f16", 256, 16, _q16("f16", False)),
    ("q16-fp8", "fp8", 256, 16, _tiled(32, False, 1, 128)),
    # 2. a tiled shape.  f32: 32 queries of ld == d would alias
    ("tiled-f32", "f32", 128, 32, _tiled(32, False, 4, 128)),
    ("tiled-f16", "f16", 256, 17, _tiled(32, False, 2, 128)),
    ("tiled-fp8", "fp8", 256, 33, _tiled(64, False, 1, 128)),
    # 3. d = 100: the per-query loop; f16 / fp8 rows are padded (ld 104 / 112)
    ("gemv-f32", "f32", 100, 3, "gemv"),
    ("gemv-f16", "f16", 100, 3, "gemv"),
    ("gemv-fp8", "fp8", 100, 3, "gemv"),
    # 4. ld != d (1120): always the copy path
    ("copy-f32", "f32", 1100, 16, _tiled(32, False, 4, 128)),
]


@pytest.mark.parametrize("label,dtype,d,nq,kernel", C_CASES, ids=[c[0] for c in C_CASES])
def test_query_pointer_forms(dev, label, dtype, d, nq, kernel):
    """The same queries from a 16-byte aligned base and from a base one float past it (every query misaligned; at
    d = 100 a query is 400 bytes, so an aligned base alone would leave them all aligned): both against the oracle,
    and bit-equal to each other."""
    from svs_amd import DeviceIndex
    n, k = 3000, 101
    m, qs = corpus_and_query("gaussian", 800 + d + nq, n, d, nq)
    idx = DeviceIndex(m, dtype=dtype)
    runs = {}
    for off in (0, 1):
        s, r, count, launches = _one_call(dev, idx, qs, k, offset=off)
        _main_kernel(launches, n, kernel)
        assert count == k
        runs[off] = (s, r)
    md, qd = _stored(idx, m, qs, dtype)
    idx.release()
    for off, (s, r) in runs.items():
        worst = check_topk(s, r, k, md, qd, f"{label} offset {off}")
        print(f"DEVBATCH C {dtype} {label} offset {off} {kernel}: max err {worst:.3g} (bound {SCORE_ATOL})")
    same_bits(runs[1], runs[0], f"{label}: misaligned vs aligned queries")


# ---- D. stream semantics ---------------------------------------------------------------------------------------------------
def _unit(nq, d, seed):
    q = np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def stream_corpus():
    m, _ = corpus_and_query("gaussian", 901, 20_000, 512, 1)
    m.setflags(write=False)
    return m


def _slow_producer(torch, tdev):
    """(a, b): operands of a matmul that keeps a stream busy for a few milliseconds, warmed up (the first call of a
    shape allocates workspace)."""
    a = torch.randn((6144, 6144), device=tdev, dtype=torch.float32)
    b = torch.mm(a, a)
    torch.cuda.synchronize(tdev)
    return a, b


def _busy(torch, a, b, times=4):
    """Enqueues the slow matmul `times` times on the current stream (0.9 TFLOP each in f32: milliseconds)."""
    for _ in range(times):
        torch.mm(a, a, out=b)


def _warm(dev, idx, nq, k, st):
    """One device call of other queries on `st`, waited for: the stream's search context exists and holds its scratch,
    so the call under test allocates nothing and its kernels are enqueued within microseconds of the call."""
    torch, tdev, _ = dev
    qb = QueryBuf(torch, tdev, _unit(nq, idx.d, 999))
    out = Outputs(torch, tdev, nq, k)
    torch.cuda.synchronize(tdev)
    assert search_device(idx, qb, k, out, st) == k
    st.synchronize()
    return out.host()


GROWTH = {
    # every call needs a larger score matrix than the one before: search_device's own guard drains the stream
    "scores-grow": [(2, 10), (40, 100), (3, 3000), (130, 50)],
    # the score matrix and the histogram are sized by the first call and never grow again; what grows later is the
    # f32 query image (64 aligned queries of ld == d are read in place, 2 take 16 rows of q16, 40 take 64; the f16
    # image of the first call serves every later one) and the SORT path's keys (2 x 32,768, then 3 x 32,768), each
    # freed with the search that reads it still queued
    "staging-and-keys-grow": [(64, 10), (2, 10), (40, 100), (2, 3000), (3, 3000)],
}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("sequence", sorted(GROWTH))
def test_scratch_growth_under_pending_work(dev, stream_corpus, dtype, sequence):
    """Calls back to back on one stream, each needing more of some scratch buffer than the one before, none waited
    for by the test: every call's records equal the host entry's.  The stream is kept busy for a few milliseconds
    first, so that each search is still queued when the next call sizes its scratch."""
    from svs_amd import DeviceIndex
    torch, tdev, _ = dev
    idx = DeviceIndex(stream_corpus, dtype=dtype)
    shapes = GROWTH[sequence]
    qs = [_unit(nq, 512, 910 + i) for i, (nq, _) in enumerate(shapes)]
    qbs = [QueryBuf(torch, tdev, q) for q in qs]
    outs = [Outputs(torch, tdev, nq, k) for nq, k in shapes]
    a, b = _slow_producer(torch, tdev)
    st = torch.cuda.Stream(device=tdev)
    torch.cuda.synchronize(tdev)
    with torch.cuda.stream(st):
        torch.mm(a, a, out=b)
    for qb, out, (_, k) in zip(qbs, outs, shapes):
        assert search_device(idx, qb, k, out, st) == k
    st.synchronize()
    for q, out, (nq, k) in zip(qs, outs, shapes):
        same_bits(out.host(), idx.search_batch(q, k), f"{dtype} nq={nq} k={k}")
    idx.release()


def test_two_streams_alternate_on_one_handle(dev, stream_corpus):
    from svs_amd import DeviceIndex
    torch, tdev, _ = dev
    idx = DeviceIndex(stream_corpus, dtype="f16")
    sts = [torch.cuda.Stream(device=tdev), torch.cuda.Stream(device=tdev)]
    qs = [_unit(17, 512, 930 + i) for i in range(8)]
    qbs = [QueryBuf(torch, tdev, q) for q in qs]
    outs = [Outputs(torch, tdev, 17, 100) for _ in qs]
    torch.cuda.synchronize(tdev)
    for i, (qb, out) in enumerate(zip(qbs, outs)):
        assert search_device(idx, qb, 100, out, sts[i % 2]) == 100
    for st in sts:
        st.synchronize()
    for i, (q, out) in enumerate(zip(qs, outs)):
        same_bits(out.host(), idx.search_batch(q, 100), f"call {i} on stream {i % 2}")
    idx.release()


def test_producer_and_consumer_are_ordered_by_the_stream(dev, stream_corpus):
    """The queries are written by a copy enqueued on the stream behind a slow kernel (the buffer holds NaN until then);
    a clone of the outputs is enqueued on the stream right behind the call.  One synchronise."""
    from svs_amd import DeviceIndex
    torch, tdev, _ = dev
    idx = DeviceIndex(stream_corpus, dtype="f32")
    q = _unit(5, 512, 940)
    qb = QueryBuf(torch, tdev, q, fill=False)
    out = Outputs(torch, tdev, 5, 100)
    a, b = _slow_producer(torch, tdev)
    st = torch.cuda.Stream(device=tdev)
    _warm(dev, idx, 5, 100, st)
    torch.cuda.synchronize(tdev)
    with torch.cuda.stream(st):
        _busy(torch, a, b)
        qb.view.copy_(qb.src, non_blocking=True)
        assert search_device(idx, qb, 100, out, st) == 100
        s2, r2 = out.s_all.clone(), out.r_all.clone()
    st.synchronize()
    exp = idx.search_batch(q, 100)
    got = out.host()
    assert np.isfinite(got[0]).all(), "NaN scores: the queries were read before their producer had run"
    same_bits(got, exp, "outputs")
    same_bits(out.host(s2, r2), exp, "clone enqueued behind the call")
    md, qd = _stored(idx, stream_corpus, q, "f32")
    idx.release()
    worst = check_topk(got[0], got[1], 100, md, qd, "producer ordering")
    print(f"DEVBATCH D f32 producer ordering: max err {worst:.3g} (bound {SCORE_ATOL})")


def test_ahead_entry_with_five_queries_waits_for_the_ready_event(dev, stream_corpus):
    """svs_index_search_device_ahead with nq = 5 is the plain call behind query_ready_event: the event is recorded on
    ANOTHER stream, behind a slow kernel and the copy that writes the queries (NaN until then)."""
    from svs_amd import DeviceIndex
    torch, tdev, _ = dev
    idx = DeviceIndex(stream_corpus, dtype="f32")
    q = _unit(5, 512, 950)
    qb = QueryBuf(torch, tdev, q, fill=False)
    out = Outputs(torch, tdev, 5, 100)
    a, b = _slow_producer(torch, tdev)
    caller, feeder = torch.cuda.Stream(device=tdev), torch.cuda.Stream(device=tdev)
    _warm(dev, idx, 5, 100, caller)
    torch.cuda.synchronize(tdev)
    with torch.cuda.stream(feeder):
        _busy(torch, a, b)
        qb.view.copy_(qb.src, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(feeder)
    assert search_device(idx, qb, 100, out, caller, ahead=True, ready=ready) == 100
    caller.synchronize()
    got = out.host()
    feeder.synchronize()
    assert np.isfinite(got[0]).all(), "NaN scores: the search did not wait for query_ready_event"
    stats = idx.ahead_stats()
    assert stats["ahead"] == 0 and stats["plain"] == 0 and stats["pipelines"] == 0, stats   # (never near a pipeline)
    plain = Outputs(torch, tdev, 5, 100)
    torch.cuda.synchronize(tdev)
    assert search_device(idx, qb, 100, plain, caller) == 100
    caller.synchronize()
    same_bits(got, plain.host(), "ahead entry vs plain device call")
    same_bits(got, idx.search_batch(q, 100), "ahead entry vs host entry")
    idx.release()


# ---- E. never fused at size --------------------------------------------------------------------------------------------------
E_CASES = [("f32", 128, _q16("f32", False)), ("f16", 256, _q16("f16", False)), ("fp8", 256, _tiled(32, False, 1, 128))]


@pytest.mark.parametrize("dtype,d,kernel", E_CASES, ids=[c[0] for c in E_CASES])
def test_never_fused_at_size(dev, dtype, d, kernel):
    from svs_amd import DeviceIndex, _native
    n, nq, k = NF1, 16, 256
    m, qs = corpus_and_query("gaussian", 7000 + d + n % 1000, n, d, nq)
    idx = DeviceIndex(m, dtype=dtype)
    s, r, count, launches = _one_call(dev, idx, qs, k)
    assert count == k
    _main_kernel(launches, n, kernel)                       # every launch over all n rows: no threshold pass
    hs, hr = idx.search_batch(qs, k)
    host_launches = _native.last_launches()
    assert host_launches[0][1] < n, f"the host entry is fused at this size (it starts with a threshold pass): {host_launches}"
    assert np.array_equal(r, hr), np.argwhere(r != hr)[:8].tolist()
    # (the fused epilogue keeps the scores its kernel computed: test_batch_kernels_gpu.py holds fused == materialised bit for bit)
    assert np.array_equal(bits(s), bits(hs)), np.argwhere(bits(s) != bits(hs))[:8].tolist()
    md, qd = _stored(idx, m, qs, dtype)
    idx.release()
    worst = check_topk(s, r, k, md, qd, f"never fused {dtype}", queries=(0, 5, 10, 15))
    print(f"DEVBATCH E {dtype} {kernel} n={n}: max err {worst:.3g} (bound {SCORE_ATOL})")


# ---- F. the Python consumer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "fp8"])
@pytest.mark.parametrize("n,k", [(3000, 7), (40, 101)], ids=["k7", "k>n"])
def test_sharded_index_search_batch_at_one_rank(dev, dtype, n, k):
    """nq * k * 4 = 84 (k = 7) and 1212 (k = 101) bytes of scores: not multiples of 8, so the row array of the record
    starts behind padding (record_layout)."""
    from svs_amd import DeviceIndex
    from svs_amd.sharded import ShardedIndex, record_layout
    torch, tdev, _ = dev
    m, qs = corpus_and_query("gaussian", 990 + n + k, n, 256, 3)
    assert record_layout(k, 3)[0] != 3 * k * 4
    idx = DeviceIndex(m, dtype=dtype)
    got = ShardedIndex(idx, idx.n, device=tdev).search_batch(qs, k)
    exp = idx.search_batch(qs, k)
    assert exp[1].shape == (3, min(k, n))
    same_bits(got, exp, f"ShardedIndex {dtype} n={n} k={k}")
    md, qd = _stored(idx, m, qs, dtype)
    idx.release()
    worst = check_topk(got[0], got[1], min(k, n), md, qd, f"ShardedIndex {dtype}")
    print(f"DEVBATCH F {dtype} n={n} k={k}: max err {worst:.3g} (bound {SCORE_ATOL})")

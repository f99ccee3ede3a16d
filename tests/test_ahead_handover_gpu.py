"""GPU: the hand-over between the run-ahead pipeline's score passes and their selection chains
(svs_index_search_device_ahead): a ring of R = 4 contexts; the last kernel of a pass carries the pass's completion
event (no record on the pass stream); the pass stream waits for a selection once per G = R / 2 passes.
svs_internal_tune(4, 1) makes pipelines with a record behind and a wait in front of every pass instead; every case
runs under both values.

Every comparison is against the SAME queries run through svs_index_search_device on the SAME index: rows equal, scores
equal as uint32.  Output slots start out as NaN / -7, so a slot nobody wrote cannot pass.
"""
import functools

import numpy as np
import pytest

from svs_amd import DeviceIndex, _native

OFF, FORCE = 11, 12     # svs_index_set_variant: never screen / screen whatever n
SENTINEL_ROW = -7
R, G = 4, 2             # AHEAD_RING, AHEAD_GROUP (svs_amd/csrc/svs_amd.hip)
M = 4 * R + 3           # searches of the ring-reuse and counter cases
KNOBS = [0, 1]
KNOB_IDS = ["carried event", "record per pass"]


def gaussian(n, d, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


@functools.lru_cache(maxsize=None)
def corpus(n, d):
    m = gaussian(n, d, 2000 + n + d)
    m.setflags(write=False)
    return m


def unit_queries(m, d, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((m, d)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(params=KNOBS, ids=KNOB_IDS)
def knob(request):
    """The hand-over of the pipelines made during the test (read when a pipeline is made)."""
    lib = _native.load()
    assert lib.svs_internal_tune(4, request.param) == 0
    yield request.param
    assert lib.svs_internal_tune(4, 0) == 0


def slots(torch, dev, m, k):
    s = torch.full((m, k), float("nan"), device=dev, dtype=torch.float32)
    r = torch.full((m, k), SENTINEL_ROW, device=dev, dtype=torch.int64)
    return s, r


def enqueue(idx, q_t, k, s, r, stream, ahead, ready=None):
    """One call per row of q_t into slot i of (s, r).  No synchronisation."""
    d = q_t.shape[1]
    for i in range(q_t.shape[0]):
        if ahead:
            idx.search_device_ahead(q_t[i].data_ptr(), 1, d, k, s[i].data_ptr(), r[i].data_ptr(), stream.cuda_stream,
                                    ready_event=ready)
        else:
            idx.search_device(q_t[i].data_ptr(), 1, d, k, s[i].data_ptr(), r[i].data_ptr(), stream.cuda_stream)


def host(s, r):
    return s.cpu().numpy().view(np.uint32), r.cpu().numpy()


def run(torch, dev, idx, q, k, ahead, stream=None):
    """All rows of q (numpy) enqueued back to back on one stream, ONE synchronise; -> (scores u32, rows) on the host."""
    q_t = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    s, r = slots(torch, dev, q.shape[0], k)
    stream = stream or torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t, k, s, r, stream, ahead)
    stream.synchronize()
    return host(s, r)


def same(got, exp, label=""):
    (gs, gr), (es, er) = got, exp
    assert not (er == SENTINEL_ROW).any(), label
    assert np.array_equal(gr, er), (label, np.argwhere(gr != er)[:8])
    assert np.array_equal(gs, es), (label, np.argwhere(gs != es)[:8])


def distinct(exp):
    assert len({tuple(row) for row in exp[1]}) == exp[1].shape[0], "every query must have an answer of its own"


def score_kernels():
    return [x for x in _native.last_launches() if x[0] != "gemv"]


# ---- 1. a pass long enough to be overtaken: four contexts, selections up to R passes behind ------------------------
@pytest.mark.gpu
def test_long_passes_24_searches_then_with_tombstones(torch_dev, knob):
    """100,000 x 1536 f32, screened by default: the pass takes tens of microseconds, as long as a selection chain, so
    passes do run beside the chains of earlier searches.  All 24 queries differ, so scratch of search i - R that
    search i found unchanged could not pass.  Then 50 rows are tombstoned, winners of every query among them: the
    mask kernel is now the last of the pass and carries the event."""
    torch, dev = torch_dev
    n, d, k = 100_000, 1536, 100
    idx = DeviceIndex(corpus(n, d), device=0)
    q = unit_queries(24, d, 3)
    exp = run(torch, dev, idx, q, k, False)
    distinct(exp)
    got = run(torch, dev, idx, q, k, True)
    launches = score_kernels()
    assert launches[0][0].startswith("gemv_f16_oneshot_kernel<") and launches[0][1:] == (n, 1), launches
    same(got, exp, "no tombstones")
    dead = sorted({int(x) for x in exp[1][:, :2].ravel()})
    dead += [x for x in range(50) if x not in dead][:50 - len(dead)]
    assert len(dead) == 50
    idx.mask_rows(dead)
    exp2 = run(torch, dev, idx, q, k, False)
    assert not np.isin(exp2[1], dead).any() and not np.array_equal(exp2[1], exp[1])
    before = idx.ahead_stats()
    same(run(torch, dev, idx, q, k, True), exp2, "50 tombstones")
    after = idx.ahead_stats()
    assert after["bound"] - before["bound"] == (24 if knob == 0 else 0), (before, after)
    idx.release()


# ---- 2. ring reuse: 4 R + 3 searches on every route -----------------------------------------------------------------
ROUTES = [
    # (label, n, d, dtype, variant, k, first score kernel)
    ("f32 screened", 12_000, 512, "f32", FORCE, 100, "gemv_f16_oneshot_kernel<"),
    ("f32 unscreened", 12_000, 512, "f32", OFF, 100, "gemv_f32_oneshot_kernel<"),
    ("f32 k=2049 (path B)", 12_000, 512, "f32", FORCE, 2049, "gemv_f32_oneshot_kernel<"),
    ("n=300 (path D)", 300, 512, "f32", 0, 100, "gemv_f32_oneshot_kernel<"),
    ("f16", 8_000, 512, "f16", 0, 100, "gemv_f16_oneshot_kernel<"),
    ("fp8", 8_000, 512, "fp8", 0, 100, "gemv_fp8_oneshot_kernel<"),
    ("f32 d=384 unrolled", 6_000, 384, "f32", 0, 100, "gemv_unrolled_kernel<"),
]


@pytest.mark.parametrize("label,n,d,dtype,variant,k,kernel", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.gpu
def test_ring_reuse_on_every_route(torch_dev, knob, label, n, d, dtype, variant, k, kernel):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(n, d), device=0, dtype=dtype)
    idx.set_variant(variant)
    q = unit_queries(M, d, 7)
    exp = run(torch, dev, idx, q, k, False)
    distinct(exp)
    got = run(torch, dev, idx, q, k, True)
    launches = score_kernels()
    assert launches and launches[0][0].startswith(kernel) and launches[0][1:] == (n, 1), (label, launches)
    same(got, exp, label)
    stats = idx.ahead_stats()
    assert stats["ahead"] == M and stats["plain"] == 0, stats
    assert stats["bound"] == (M if knob == 0 else 0), stats     # every route launches its last kernel with the event
    idx.release()


# ---- 3. what the calls put on the pass stream -----------------------------------------------------------------------
@pytest.mark.gpu
def test_counters_on_a_fresh_index(torch_dev, knob):
    """M calls, no ready event, timing off.  Carried event: every pass's event is bound to a launch, nothing is
    recorded on the pass stream, and the stream waits at the passes i in [R, M) with i % G == 0.  Record per pass:
    one record per pass and a wait in front of every pass from the R-th on."""
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(M, 512, 11)
    exp = run(torch, dev, idx, q, 100, False)
    assert idx.ahead_stats() == {"ahead": 0, "plain": 0, "handed_over": 0, "pipelines": 0, "bound": 0, "pass_records": 0,
                                 "pass_waits": 0}
    same(run(torch, dev, idx, q, 100, True), exp)
    stats = idx.ahead_stats()
    assert stats["ahead"] == M and stats["pipelines"] == 1, stats
    if knob == 0:
        assert stats["bound"] == M and stats["pass_records"] == 0, stats
        assert stats["pass_waits"] == len([i for i in range(R, M) if i % G == 0]), stats
    else:
        assert stats["bound"] == 0 and stats["pass_records"] == M, stats
        assert stats["pass_waits"] == M - R, stats
    idx.release()


# ---- 4. timing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_timed_steps(torch_dev, knob, variant):
    """On a timed step `e1` is the event the pass's last kernel carries and the caller's stream waits for."""
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q = unit_queries(6, 512, 13)
    exp = run(torch, dev, idx, q, 100, False)
    idx.set_timing(1)
    got = run(torch, dev, idx, q, 100, True)
    score_ms, select_ms, launches = idx.get_timing()
    idx.set_timing(0)
    print(f"knob {knob} variant {variant}: score {score_ms:.5f} ms, select {select_ms:.5f} ms over {launches} searches")
    same(got, exp)
    assert launches == 6
    assert np.isfinite(score_ms) and np.isfinite(select_ms)
    assert score_ms > 0.0
    stats = idx.ahead_stats()
    assert stats["bound"] == (6 if knob == 0 else 0), stats
    idx.release()


# ---- 5. the ring's contexts get their scratch together: no call after the first allocates ---------------------------
@pytest.mark.parametrize("n,k,variant", [(300, 100, 0), (12_000, 2049, 0), (12_000, 100, FORCE)],
                         ids=["path D", "path B", "screened"])
@pytest.mark.gpu
def test_no_call_after_the_first_blocks_the_host(torch_dev, knob, n, k, variant):
    """ONE warm-up call, then R + 2 calls behind a ready event that a busy stream has not reached yet: every call
    returns while the event is still pending (a call that drained the pipeline to grow a context's scratch would have
    waited for it), and the results are the plain ones."""
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(n, 512), device=0)
    idx.set_variant(variant)
    m = R + 2
    q = unit_queries(m, 512, 17)
    exp = run(torch, dev, idx, q, k, False)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, m, k)
    caller, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    same(run(torch, dev, idx, q[:1], k, True, caller), (exp[0][:1], exp[1][:1]), "warm-up")
    with torch.cuda.stream(feeder):
        torch.cuda._sleep(100_000_000)                   # tens of milliseconds; the calls below take well under one
        ready = torch.cuda.Event()
        ready.record(feeder)
    enqueue(idx, q_t, k, s, r, caller, True, ready=ready)
    assert not ready.query(), "a call blocked until the ready event had fired"
    caller.synchronize()
    same(host(s, r), exp)
    idx.release()


# ---- 6. drains ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_append_past_the_capacity_between_two_runs(torch_dev, knob):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    m = R + 1
    q = unit_queries(2 * m, 512, 19)
    before = run(torch, dev, idx, q[:m], 100, False)
    extra = gaussian(3_000, 512, 20)
    extra[5:5 + m] = q[m:]                               # the new best rows of the later calls
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 2 * m, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t[:m], 100, s[:m], r[:m], st, True)
    idx.append(extra)                                    # (no spare capacity: the rows and the shadow move, the scores grow)
    assert idx.n == 15_000
    enqueue(idx, q_t[m:], 100, s[m:], r[m:], st, True)
    st.synchronize()
    after = run(torch, dev, idx, q[m:], 100, False)
    assert after[1][:, 0].tolist() == [12_005 + i for i in range(m)]
    su, rr = host(s, r)
    same((su[:m], rr[:m]), before, "enqueued before the append")
    same((su[m:], rr[m:]), after, "enqueued after the append")
    idx.release()


@pytest.mark.gpu
def test_set_screen_between_calls(torch_dev, knob):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    m = R + 1
    q = unit_queries(3 * m, 512, 23)
    exp = run(torch, dev, idx, q, 100, False)
    distinct(exp)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 3 * m, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t[:m], 100, s[:m], r[:m], st, True)
    idx.set_screen(0)
    assert idx.screen_stats()["shadow"] == 0
    enqueue(idx, q_t[m:2 * m], 100, s[m:2 * m], r[m:2 * m], st, True)
    assert _native.last_launches()[-1][0].startswith("gemv_f32_oneshot_kernel<")
    idx.set_screen(1)
    assert idx.screen_stats()["shadow"] == 1
    enqueue(idx, q_t[2 * m:], 100, s[2 * m:], r[2 * m:], st, True)
    assert _native.last_launches()[0][0].startswith("gemv_f16_oneshot_kernel<")
    st.synchronize()
    same(host(s, r), exp)
    idx.release()


@pytest.mark.gpu
def test_release_with_two_rings_of_searches_enqueued(torch_dev, knob):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(2 * R, 512, 29)
    exp = run(torch, dev, idx, q, 100, False)
    distinct(exp)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 2 * R, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t, 100, s, r, st, True)
    idx.release()                                        # the only owner: the library drains what it enqueued
    torch.cuda.synchronize(dev)
    same(host(s, r), exp)

"""GPU: svs_index_search_device_ahead (the run-ahead device entry: score passes one after another on a stream of the
library's own, each search's selection chain on the caller's stream beside the next pass) returns what
svs_index_search_device returns.

Every comparison below is against the SAME queries run through svs_index_search_device on the SAME index: rows must be
equal and scores equal as uint32.  Output slots start out as NaN / -7, so a slot nobody wrote cannot pass.
"""
import functools
import threading

import numpy as np
import pytest

from svs_amd import DeviceIndex, _native

OFF, FORCE = 11, 12     # svs_index_set_variant: never screen / screen whatever n
SENTINEL_ROW = -7


def gaussian(n, d, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


@functools.lru_cache(maxsize=None)
def corpus(n, d):
    m = gaussian(n, d, 1000 + n + d)
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


def slots(torch, dev, m, k):
    s = torch.full((m, k), float("nan"), device=dev, dtype=torch.float32)
    r = torch.full((m, k), SENTINEL_ROW, device=dev, dtype=torch.int64)
    return s, r


def enqueue(idx, q_t, k, s, r, stream, how, ready=None):
    """One call per row of q_t into slot i of (s, r); how(i) -> 'ahead' | 'plain'.  No synchronisation."""
    d = q_t.shape[1]
    for i in range(q_t.shape[0]):
        if how(i) == "ahead":
            idx.search_device_ahead(q_t[i].data_ptr(), 1, d, k, s[i].data_ptr(), r[i].data_ptr(), stream.cuda_stream,
                                    ready_event=ready)
        else:
            idx.search_device(q_t[i].data_ptr(), 1, d, k, s[i].data_ptr(), r[i].data_ptr(), stream.cuda_stream)


def run(torch, dev, idx, q, k, how, stream=None):
    """All rows of q (numpy) enqueued back to back on one stream, ONE synchronise; -> (scores u32, rows) on the host."""
    q_t = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    s, r = slots(torch, dev, q.shape[0], k)
    stream = stream or torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t, k, s, r, stream, how)
    stream.synchronize()
    return s.cpu().numpy().view(np.uint32), r.cpu().numpy()


def plain(torch, dev, idx, q, k):
    return run(torch, dev, idx, q, k, lambda i: "plain")


def ahead(torch, dev, idx, q, k, stream=None):
    return run(torch, dev, idx, q, k, lambda i: "ahead", stream)


def same(got, exp, label=""):
    (gs, gr), (es, er) = got, exp
    assert not (er == SENTINEL_ROW).any(), label
    assert np.array_equal(gr, er), (label, np.argwhere(gr != er)[:8])
    assert np.array_equal(gs, es), (label, np.argwhere(gs != es)[:8])


# ---- 1. every route, 24 searches ahead ------------------------------------------------------------------------------
ROUTES = [
    # (label, n, d, dtype, variant, k, first score kernel)
    ("f32 screened k=100", 12_000, 512, "f32", FORCE, 100, "gemv_f16_oneshot_kernel<"),
    ("f32 screened k=1", 12_000, 512, "f32", FORCE, 1, "gemv_f16_oneshot_kernel<"),
    ("f32 k=2049 (path B)", 12_000, 512, "f32", FORCE, 2049, "gemv_f32_oneshot_kernel<"),
    ("f32 d=384 unrolled", 6_000, 384, "f32", 0, 100, "gemv_unrolled_kernel<"),
    ("f16", 8_000, 512, "f16", 0, 100, "gemv_f16_oneshot_kernel<"),
    ("fp8", 8_000, 512, "fp8", 0, 100, "gemv_fp8_oneshot_kernel<"),
    ("n=300 (path D)", 300, 512, "f32", 0, 100, "gemv_f32_oneshot_kernel<"),
]


@pytest.mark.parametrize("label,n,d,dtype,variant,k,kernel", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.gpu
def test_every_route_24_ahead(torch_dev, label, n, d, dtype, variant, k, kernel):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(n, d), device=0, dtype=dtype)
    idx.set_variant(variant)
    q = unit_queries(24, d, 7)
    exp = plain(torch, dev, idx, q, k)
    got = ahead(torch, dev, idx, q, k)
    launches = [x for x in _native.last_launches() if x[0] != "gemv"]
    assert launches and launches[0][0].startswith(kernel) and launches[0][1:] == (n, 1), (label, launches)
    same(got, exp, label)
    assert len({tuple(row) for row in exp[1]}) > 1, "the queries must have different answers"
    idx.release()


# ---- 2. scratch reuse: q, -q, q, ... on the two alternating contexts ------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_alternating_queries_do_not_share_scratch(torch_dev, variant):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q0 = unit_queries(1, 512, 11)[0]
    q = np.stack([q0 if i % 2 == 0 else -q0 for i in range(64)])
    exp = plain(torch, dev, idx, q, 100)
    assert not np.intersect1d(exp[1][0], exp[1][1]).size, "q and -q must share no winner"
    same(ahead(torch, dev, idx, q, 100), exp)
    idx.release()


# ---- 3. query_ready_event --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_query_ready_event_orders_the_score_pass(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(2, 512, 13)
    exp = plain(torch, dev, idx, q[:1], 100)
    src = torch.from_numpy(q[:1].copy()).to(dev)
    qbuf = torch.from_numpy(q[1:2].copy()).to(dev)       # (holds ANOTHER query until the copy below has run)
    s, r = slots(torch, dev, 1, 100)
    caller, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(feeder):
        torch.cuda._sleep(40_000_000)                    # keeps the feeding stream busy for some milliseconds
        qbuf.copy_(src, non_blocking=True)
        ready = torch.cuda.Event()
        ready.record(feeder)
    enqueue(idx, qbuf, 100, s, r, caller, lambda i: "ahead", ready=ready)
    caller.synchronize()
    same((s.cpu().numpy().view(np.uint32), r.cpu().numpy()), exp)
    feeder.synchronize()
    idx.release()


# ---- 4. results are ordered on the caller's stream -----------------------------------------------------------------
@pytest.mark.gpu
def test_work_enqueued_after_the_call_sees_the_result(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(6, 512, 17)
    exp = plain(torch, dev, idx, q, 100)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 6, 100)
    s2, r2 = slots(torch, dev, 6, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(st):
        for i in range(6):
            enqueue(idx, q_t[i:i + 1], 100, s[i:i + 1], r[i:i + 1], st, lambda _: "ahead")
            s2[i].copy_(s[i], non_blocking=True)         # device to device, right behind the call
            r2[i].copy_(r[i], non_blocking=True)
    st.synchronize()
    same((s2.cpu().numpy().view(np.uint32), r2.cpu().numpy()), exp)
    idx.release()


# ---- 5. mixing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_ahead_plain_ahead_on_one_stream(torch_dev, variant):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q = unit_queries(9, 512, 19)
    exp = plain(torch, dev, idx, q, 100)
    same(run(torch, dev, idx, q, 100, lambda i: "plain" if i % 3 == 1 else "ahead"), exp)
    idx.release()


@pytest.mark.gpu
def test_two_threads_two_streams_one_handle(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    qs = [unit_queries(16, 512, 23), unit_queries(16, 512, 29)]
    exps = [plain(torch, dev, idx, q, 100) for q in qs]
    streams = [torch.cuda.Stream(device=dev) for _ in qs]
    got, errs = [None, None], []

    def work(t):
        try:
            got[t] = ahead(torch, dev, idx, qs[t], 100, streams[t])
        except Exception as e:  # noqa: BLE001 -- reported by the assertion below
            errs.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(2):
        same(got[t], exps[t], f"thread {t}")
    idx.release()


# ---- 6. ingest between calls, no synchronise in between -----------------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_mask_between_calls(torch_dev, variant):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q = np.repeat(unit_queries(1, 512, 31), 8, axis=0)
    before = plain(torch, dev, idx, q[:4], 100)
    winner = int(before[1][0, 0])
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 8, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t[:4], 100, s[:4], r[:4], st, lambda i: "ahead")
    idx.mask_rows([winner])
    enqueue(idx, q_t[4:], 100, s[4:], r[4:], st, lambda i: "ahead")
    st.synchronize()
    after = plain(torch, dev, idx, q[4:], 100)
    assert winner not in after[1]
    su, rr = s.cpu().numpy().view(np.uint32), r.cpu().numpy()
    same((su[:4], rr[:4]), before, "enqueued before the mask")
    same((su[4:], rr[4:]), after, "enqueued after the mask")
    idx.release()


@pytest.mark.gpu
def test_append_past_the_capacity_between_calls(torch_dev):
    torch, dev = torch_dev
    base = corpus(12_000, 512)
    idx = DeviceIndex(base, device=0)
    idx.set_variant(FORCE)
    q1 = unit_queries(1, 512, 37)
    q = np.repeat(q1, 8, axis=0)
    before = plain(torch, dev, idx, q[:4], 100)
    extra = gaussian(3_000, 512, 38)
    extra[5] = q1[0]                                     # the new best row of every later call
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 8, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t[:4], 100, s[:4], r[:4], st, lambda i: "ahead")
    idx.append(extra)                                    # (no spare capacity: the rows and the shadow move)
    assert idx.n == 15_000
    enqueue(idx, q_t[4:], 100, s[4:], r[4:], st, lambda i: "ahead")
    st.synchronize()
    after = plain(torch, dev, idx, q[4:], 100)
    assert after[1][0, 0] == 12_005
    su, rr = s.cpu().numpy().view(np.uint32), r.cpu().numpy()
    same((su[:4], rr[:4]), before, "enqueued before the append")
    same((su[4:], rr[4:]), after, "enqueued after the append")
    idx.release()


@pytest.mark.gpu
def test_set_screen_between_calls(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(12, 512, 41)
    exp = plain(torch, dev, idx, q, 100)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 12, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t[:4], 100, s[:4], r[:4], st, lambda i: "ahead")
    idx.set_screen(0)
    assert idx.screen_stats()["shadow"] == 0
    enqueue(idx, q_t[4:8], 100, s[4:8], r[4:8], st, lambda i: "ahead")
    assert _native.last_launches()[-1][0].startswith("gemv_f32_oneshot_kernel<")
    idx.set_screen(1)
    assert idx.screen_stats()["shadow"] == 1
    enqueue(idx, q_t[8:], 100, s[8:], r[8:], st, lambda i: "ahead")
    assert _native.last_launches()[0][0].startswith("gemv_f16_oneshot_kernel<")
    st.synchronize()
    same((s.cpu().numpy().view(np.uint32), r.cpu().numpy()), exp)
    idx.release()


# ---- 7. release with searches enqueued ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_release_with_searches_enqueued(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(16, 512, 43)
    exp = plain(torch, dev, idx, q, 100)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 16, 100)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    enqueue(idx, q_t, 100, s, r, st, lambda i: "ahead")
    idx.release()                                        # the only owner: the library drains what it enqueued
    torch.cuda.synchronize(dev)
    same((s.cpu().numpy().view(np.uint32), r.cpu().numpy()), exp)


# ---- 8. introspection ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_launch_record_timing_and_screen_counters(torch_dev, variant):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q = unit_queries(6, 512, 47)
    plain(torch, dev, idx, q[:1], 100)
    rec_plain = _native.last_launches()
    ahead(torch, dev, idx, q[:1], 100)
    assert _native.last_launches() == rec_plain and rec_plain
    torch.cuda.synchronize(dev)
    before = idx.screen_stats()
    idx.set_timing(1)
    ahead(torch, dev, idx, q, 100)
    score_ms, select_ms, launches = idx.get_timing()
    idx.set_timing(0)
    print(f"variant {variant}: score {score_ms:.4f} ms, select {select_ms:.4f} ms over {launches} searches")
    assert launches == 6
    assert np.isfinite(score_ms) and np.isfinite(select_ms) and score_ms >= 0.0 and select_ms >= 0.0
    after = idx.screen_stats()
    assert after["screened"] - before["screened"] == (6 if variant == FORCE else 0), (before, after)
    assert after["fallback"] == before["fallback"]
    idx.release()


# ---- 9. ShardedIndex, one rank --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [FORCE, OFF], ids=["screened", "unscreened"])
@pytest.mark.gpu
def test_sharded_index_one_rank_enqueues_ahead(torch_dev, variant):
    torch, dev = torch_dev
    from svs_amd.sharded import ShardedIndex
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(variant)
    q = unit_queries(20, 512, 53)
    sh = ShardedIndex(idx, idx.n, device=dev, streams=1)
    assert sh.runs_ahead
    sh.open(20, 100)
    q_t = torch.from_numpy(q).to(dev)
    torch.cuda.synchronize(dev)
    for i in range(20):
        assert sh.enqueue(q_t[i].data_ptr(), 512) == i
    res = sh.collect()
    assert len(res) == 20
    for i in range(20):
        exp = idx.search(q[i], 100)
        assert res[i][1].tolist() == [row for _, row in exp], i
        assert res[i][0].view(np.uint32).tolist() == np.array([s for s, _ in exp], dtype=np.float32).view(np.uint32).tolist(), i
    idx.release()


# ---- 10. pipelines are per caller stream, four per index: streams that come and go keep running ahead ----------------
@pytest.mark.gpu
def test_more_than_four_streams_in_sequence_still_run_ahead(torch_dev):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(4, 512, 59)
    exp = plain(torch, dev, idx, q, 100)
    streams = [torch.cuda.Stream(device=dev) for _ in range(10)]
    assert len({s.cuda_stream for s in streams}) == 10
    for n_used, st in enumerate(streams, 1):
        same(ahead(torch, dev, idx, q, 100, st), exp, f"stream {n_used}")     # (synchronises: the pipeline is idle after)
        stats = idx.ahead_stats()
        assert stats["plain"] == 0 and stats["ahead"] == 4 * n_used, stats
        assert stats["pipelines"] == min(n_used, 4) and stats["handed_over"] == max(n_used - 4, 0), stats
    same(ahead(torch, dev, idx, q, 100, streams[0]), exp, "the first stream again")
    assert idx.ahead_stats()["plain"] == 0
    idx.release()


@pytest.mark.gpu
def test_sharded_index_reopened_and_rebuilt_still_runs_ahead(torch_dev):
    torch, dev = torch_dev
    from svs_amd.sharded import ShardedIndex
    idx = DeviceIndex(corpus(12_000, 512), device=0)
    idx.set_variant(FORCE)
    q = unit_queries(3, 512, 61)
    exp = plain(torch, dev, idx, q, 100)
    q_t = torch.from_numpy(q).to(dev)
    torch.cuda.synchronize(dev)
    calls = 0
    for obj in range(6):                                  # six objects on one index, each opened twice
        sh = ShardedIndex(idx, idx.n, device=dev, streams=1)
        for _ in range(2):
            sh.open(3, 100)
            for i in range(3):
                sh.enqueue(q_t[i].data_ptr(), 512)
            res = sh.collect()
            calls += 3
            for i in range(3):
                assert np.array_equal(res[i][1], exp[1][i]) and np.array_equal(res[i][0].view(np.uint32), exp[0][i]), (obj, i)
            stats = idx.ahead_stats()
            assert stats["plain"] == 0 and stats["ahead"] == calls, stats
    assert idx.ahead_stats()["pipelines"] <= 4
    idx.release()


# ---- 11. routes without the window path (path B, path D) run ahead too: no call waits on the host ------------------
@pytest.mark.parametrize("n,k", [(300, 100), (12_000, 2049)], ids=["path D", "path B"])
@pytest.mark.gpu
def test_routes_without_window_scratch_do_not_block_the_host(torch_dev, n, k):
    """Eight calls behind a ready event that a busy stream has not reached yet: every call returns while the event is
    still pending (a call that drained the pipeline first would have waited for it), and the results are the plain ones."""
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(n, 512), device=0)
    q = unit_queries(8, 512, 67)
    exp = plain(torch, dev, idx, q, k)
    q_t = torch.from_numpy(q).to(dev)
    s, r = slots(torch, dev, 8, k)
    caller, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    same(ahead(torch, dev, idx, q[:2], k, caller), (exp[0][:2], exp[1][:2]), "warm-up")   # both contexts have their scratch
    with torch.cuda.stream(feeder):
        torch.cuda._sleep(100_000_000)                   # tens of milliseconds; the eight calls below take well under one
        ready = torch.cuda.Event()
        ready.record(feeder)
    enqueue(idx, q_t, k, s, r, caller, lambda i: "ahead", ready=ready)
    assert not ready.query(), "a call blocked until the ready event had fired"
    caller.synchronize()
    same((s.cpu().numpy().view(np.uint32), r.cpu().numpy()), exp)
    idx.release()


# ---- 12. a ready event that guards nothing is refused ---------------------------------------------------------------
@pytest.mark.gpu
def test_unrecorded_ready_event_is_refused(torch_dev):
    torch, dev = torch_dev
    from svs_amd.sharded import ShardedIndex
    idx = DeviceIndex(corpus(300, 512), device=0)
    q_t = torch.from_numpy(unit_queries(1, 512, 71)).to(dev)
    s, r = slots(torch, dev, 1, 10)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with pytest.raises(ValueError):
        enqueue(idx, q_t, 10, s, r, st, lambda i: "ahead", ready=torch.cuda.Event())
    sh = ShardedIndex(idx, idx.n, device=dev, streams=2)   # (two streams: the alternating path, which waits through torch)
    assert not sh.runs_ahead
    sh.open(2, 10)
    with pytest.raises(ValueError):
        sh.enqueue(q_t[0].data_ptr(), 512, ready_event=torch.cuda.Event())
    with pytest.raises(TypeError):
        sh.enqueue(q_t[0].data_ptr(), 512, ready_event=12345)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    sh.enqueue(q_t[0].data_ptr(), 512, ready_event=done)
    assert len(sh.collect()) == 1
    st.synchronize()
    assert (r.cpu().numpy() == SENTINEL_ROW).all()        # the refused call enqueued nothing
    idx.release()

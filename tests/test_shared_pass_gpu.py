"""GPU: shared corpus passes of the run-ahead pipeline (svs_amd/csrc/pass_share.h; svs_index_search_device_ahead).

Single-query searches queued on one pipeline are served by ONE pass over the half rows when their queries are already
complete as that pass starts.  Every case compares all results, rows and uint32 score bits, with the same queries
through svs_index_search_device, and checks the claim kernels' counters against a small host model of the claim rule.

A backlog is made without any hook: the first search of a run carries a ready event that is recorded on a side stream
behind torch.cuda._sleep (tens of milliseconds); the searches enqueued after it, without events, are all published
before pass 0 runs.  Every index does ONE warm-up call first (the ring's scratch is allocated there), which the model
sees as a search of an earlier batch.
"""
import functools
import os
import re

import numpy as np
import pytest

from svs_amd import DeviceIndex, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, FORCE = 11, 12     # svs_index_set_variant: never screen / screen whatever n
SENTINEL_ROW = -7
SLEEP_CYCLES = 60_000_000     # tens of milliseconds; enqueuing a backlog takes about one


# ---- the rule's constants, read from the source ----------------------------------------------------------------------
def _const(path, name):
    with open(os.path.join(ROOT, "svs_amd", "csrc", path)) as f:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


RING = _const("svs_amd.hip", "AHEAD_RING")
GROUP = _const("svs_amd.hip", "AHEAD_GROUP")
LAG = _const("svs_amd.hip", "AHEAD_LAG")
SHARE_MAX = _const("pass_share.h", "SHARE_MAX")
SHARE_DEFAULT = _const("pass_share.h", "SHARE_DEFAULT")
MAILBOX_SIZE = _const("pass_share.h", "MAILBOX_SIZE")
SHARE_NSTEP_MAX = _const("gemv_f16.h", "F16_SHARE_NSTEP_MAX")      # rows of up to this many 512-half steps share


# ---- the host model of the claim rule --------------------------------------------------------------------------------
def covered_before(i):
    """Selections [0, covered) are over for everything on the pass stream from pass i on: the wait rule of AheadPipe
    (searches counted from the last drain).  The pass stream waits at the passes i >= LAG with i % GROUP == 0, for the
    selection of search i - LAG."""
    g = i - i % GROUP
    return g - LAG + 1 if g >= LAG else 0


def reach_of(i):
    """The last search whose context pass i may write."""
    return covered_before(i) + RING - 1


def claim_model(searches, limit):
    """searches: dicts in call order since the last drain -- share (the search publishes and its pass asks the claim
    kernel), claimable, key (what its pass reads: equal keys share), batch (published before the passes of the same
    batch run, after those of earlier ones).  -> passes that served [0, 1, 2, ...] searches."""
    hist = [0] * (SHARE_MAX + 1)
    served = 0
    for i, s in enumerate(searches):
        if not s["share"]:
            continue
        if served > i:
            hist[0] += 1
            continue
        c = 1
        while c < limit:
            t = i + c
            if t >= len(searches) or t > reach_of(i):
                break
            o = searches[t]
            if not (o["share"] and o["claimable"] and o["key"] == s["key"] and o["batch"] == s["batch"]):
                break
            c += 1
        served = i + c
        hist[c] += 1
    return hist


def counters_of(hist):
    return {"shared_passes": sum(hist[2:]), "claimed": sum((c - 1) * h for c, h in enumerate(hist) if c >= 2),
            "empty_passes": hist[0]}


def S(batch, share=True, claimable=True, key=0):
    return {"share": share, "claimable": claimable, "key": key, "batch": batch}


def backlog_model(m, first=1):
    """The warm-up call, then m searches of which the first carries the ready event."""
    return [S(0)] * first + [S(1, claimable=False)] + [S(1)] * (m - 1)


# ---- plumbing ---------------------------------------------------------------------------------------------------------
def gaussian(n, d, seed):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


@functools.lru_cache(maxsize=4)
def corpus(n, d):
    m = gaussian(n, d, 3000 + n + d)
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


@pytest.fixture
def share_limit():
    """svs_internal_tune(5, v) for the pipelines made during the test; the default afterwards."""
    lib = _native.load()

    def set_limit(v):
        assert lib.svs_internal_tune(5, v) == 0
    yield set_limit
    assert lib.svs_internal_tune(5, SHARE_DEFAULT) == 0


def slots(torch, dev, m, k):
    s = torch.full((m, k), float("nan"), device=dev, dtype=torch.float32)
    r = torch.full((m, k), SENTINEL_ROW, device=dev, dtype=torch.int64)
    return s, r


def host(s, r):
    return s.cpu().numpy().view(np.uint32), r.cpu().numpy()


def call(idx, q_row, k, s_row, r_row, stream, ahead=True, ready=None):
    d = q_row.shape[0]
    if ahead:
        idx.search_device_ahead(q_row.data_ptr(), 1, d, k, s_row.data_ptr(), r_row.data_ptr(), stream.cuda_stream, ready_event=ready)
    else:
        idx.search_device(q_row.data_ptr(), 1, d, k, s_row.data_ptr(), r_row.data_ptr(), stream.cuda_stream)


def plain(torch, dev, idx, q_t, k):
    """q_t: device tensor (m, d), or a list of (query row, k)."""
    items = [(q_t[i], k) for i in range(q_t.shape[0])] if k is not None else q_t
    kmax = max(kk for _, kk in items)
    s, r = slots(torch, dev, len(items), kmax)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    for i, (row, kk) in enumerate(items):
        call(idx, row, kk, s[i], r[i], st, ahead=False)
    st.synchronize()
    return host(s, r)


def sleeping_event(torch, dev, feeder):
    with torch.cuda.stream(feeder):
        torch.cuda._sleep(SLEEP_CYCLES)
        ev = torch.cuda.Event()
        ev.record(feeder)
    return ev


def backlog(torch, dev, idx, items, stream, feeder, events=()):
    """items: (query row, k) in call order, all ahead on `stream`; item 0 carries a sleeping ready event, the items named
    in `events` an event that has fired already.  Every call returns while the event is pending.  -> (scores u32, rows)."""
    kmax = max(kk for _, kk in items)
    s, r = slots(torch, dev, len(items), kmax)
    fired = torch.cuda.Event()
    fired.record(feeder)
    feeder.synchronize()
    ev = sleeping_event(torch, dev, feeder)
    for i, (row, kk) in enumerate(items):
        call(idx, row, kk, s[i], r[i], stream, ready=ev if i == 0 else (fired if i in events else None))
    assert not ev.query(), "the backlog was not enqueued while the first search's event was pending"
    stream.synchronize()
    return host(s, r)


def same(got, exp, label=""):
    (gs, gr), (es, er) = got, exp
    assert not (er == SENTINEL_ROW).any(), label
    assert np.array_equal(gr, er), (label, np.argwhere(gr != er)[:8])
    assert np.array_equal(gs, es), (label, np.argwhere(gs != es)[:8])


def shared_stats(idx):
    st = idx.ahead_stats(shared=True)
    return {k: st[k] for k in ("shared_passes", "claimed", "empty_passes")}


def warm_up(torch, dev, idx, q_row, k, stream):
    s, r = slots(torch, dev, 1, k)
    call(idx, q_row, k, s[0], r[0], stream)
    stream.synchronize()
    return host(s, r)


def make(torch, dev, dtype="f32", n=12_000, d=512, variant=FORCE):
    if dtype == "f16":
        n, variant = 8_000, 0
    idx = DeviceIndex(corpus(n, d), device=0, dtype=dtype)
    idx.set_variant(variant)
    return idx, torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)


DTYPES = ["f32", "f16"]


# ---- 1. backlog lengths -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, SHARE_DEFAULT, SHARE_DEFAULT + 1, 2 * RING + 3])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.gpu
def test_backlog_lengths(torch_dev, dtype, m):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev, dtype)
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 5 + m)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    assert len({tuple(row) for row in exp[1]}) == m + 1, "every query must have an answer of its own"
    same(warm_up(torch, dev, idx, q_t[0], 100, st), (exp[0][:1], exp[1][:1]), "warm-up")
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    same(got, (exp[0][1:], exp[1][1:]), f"backlog of {m}")
    want = counters_of(claim_model(backlog_model(m), SHARE_DEFAULT))
    print(f"{dtype} backlog {m}: {shared_stats(idx)} (model {want})")
    assert shared_stats(idx) == want
    if m <= SHARE_DEFAULT + 1:          # (the first search's pass serves as many as it may; a search left over is alone)
        assert want["claimed"] == min(m, SHARE_DEFAULT) - 1
    else:
        assert want["claimed"] >= m // 2
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.gpu
def test_limit_one_claims_nothing(torch_dev, share_limit, dtype):
    torch, dev = torch_dev
    share_limit(1)
    idx, st, feeder = make(torch, dev, dtype)
    m = 2 * RING + 3
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 31)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    same(backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder), (exp[0][1:], exp[1][1:]))
    assert shared_stats(idx) == {"shared_passes": 0, "claimed": 0, "empty_passes": 0}
    idx.release()


@pytest.mark.parametrize("limit", [2, 3])
@pytest.mark.gpu
def test_smaller_limits(torch_dev, share_limit, limit):
    torch, dev = torch_dev
    share_limit(limit)
    idx, st, feeder = make(torch, dev)
    m = RING + 3
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 37)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    same(backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder), (exp[0][1:], exp[1][1:]))
    assert shared_stats(idx) == counters_of(claim_model(backlog_model(m), limit))
    idx.release()


# ---- 2. every shadow row geometry, with and without a clamped tail ---------------------------------------------------
@pytest.mark.parametrize("n", [12_000, 12_001])
@pytest.mark.parametrize("d", list(range(512, 4097, 512)))
@pytest.mark.gpu
def test_row_geometries(torch_dev, d, n):
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(12_001, d)[:n], device=0)
    idx.set_variant(FORCE)
    st, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    m = SHARE_DEFAULT + 2
    q_t = torch.from_numpy(unit_queries(m + 1, d, 41)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    launches = [x for x in _native.last_launches() if x[0] != "gemv"]
    assert launches[0][0].startswith(f"gemv_f16_oneshot_kernel<{d // 512},") and launches[0][1:] == (n, 1), launches
    same(got, (exp[0][1:], exp[1][1:]), f"d={d} n={n}")
    if d // 512 <= SHARE_NSTEP_MAX:
        want = counters_of(claim_model(backlog_model(m), SHARE_DEFAULT))
        assert want["claimed"] == SHARE_DEFAULT
    else:   # sharing is off for this row length
        want = {"shared_passes": 0, "claimed": 0, "empty_passes": 0}
    assert shared_stats(idx) == want, (d, n)
    idx.release()


# ---- 3. non-finite values between ordinary queries of one shared pass ------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.gpu
def test_non_finite_queries_between_neighbours(torch_dev, dtype):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev, dtype)
    q = unit_queries(2 * SHARE_DEFAULT + 1, 512, 43)
    q[2, 17] = np.nan                   # (between 1 and 3 in the pass of search 1)
    q[6] *= np.float32(1e30)            # (a query that overflows half)
    q_t = torch.from_numpy(q).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    m = q.shape[0] - 1
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    same(got, (exp[0][1:], exp[1][1:]))
    assert shared_stats(idx) == counters_of(claim_model(backlog_model(m), SHARE_DEFAULT))
    idx.release()


# ---- 4. what is not claimable -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.gpu
def test_timed_searches_are_never_claimed(torch_dev, every):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = 2 * RING + 1
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 47)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    idx.set_timing(every)               # (the step counter starts over: backlog searches 0, every, 2 every ... are timed)
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    score_ms, select_ms, timed = idx.get_timing()
    idx.set_timing(0)
    same(got, (exp[0][1:], exp[1][1:]))
    assert timed == len(range(0, m, every)) and score_ms > 0.0
    model = [S(0)] + [S(1, claimable=(i > 0 and i % every != 0)) for i in range(m)]
    want = counters_of(claim_model(model, SHARE_DEFAULT))
    assert shared_stats(idx) == want
    assert (want["claimed"] == 0) == (every == 1)
    idx.release()


@pytest.mark.gpu
def test_a_ready_event_in_the_middle_is_not_claimed(torch_dev):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = 7
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 53)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder, events={2})
    same(got, (exp[0][1:], exp[1][1:]))
    model = [S(0)] + [S(1, claimable=i not in (0, 2)) for i in range(m)]
    want = counters_of(claim_model(model, SHARE_DEFAULT))
    assert want["claimed"] == 1 + 3     # (1 by the first search, 3 by the one with the event)
    assert shared_stats(idx) == want
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.gpu
def test_path_b_between_shared_searches(torch_dev, dtype):
    """k = 2049 takes the sort path: its search is served by its own pass and ends the run an earlier pass may claim."""
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev, dtype)
    ks = [100, 100, 2049, 100, 100, 100]
    q_t = torch.from_numpy(unit_queries(len(ks) + 2, 512, 59)).to(dev)
    items = [(q_t[2 + i], kk) for i, kk in enumerate(ks)]
    exp = plain(torch, dev, idx, items, None)
    st_w = warm_up(torch, dev, idx, q_t[0], 2049, st)     # (the ring's sort keys are allocated here, not in the backlog)
    assert st_w[1].shape == (1, 2049)
    warm_up(torch, dev, idx, q_t[1], 100, st)
    got = backlog(torch, dev, idx, items, st, feeder)
    for i, kk in enumerate(ks):
        same((got[0][i:i + 1, :kk], got[1][i:i + 1, :kk]), (exp[0][i:i + 1, :kk], exp[1][i:i + 1, :kk]), f"search {i}, k={kk}")
    # (the second warm-up call found no window scratch in the ring: it drained the pipeline and is search 0 of the model)
    model = [S(0)] + [S(1, share=kk == 100, claimable=i > 0) for i, kk in enumerate(ks)]
    want = counters_of(claim_model(model, SHARE_DEFAULT))
    assert want["claimed"] == 1 + 2
    assert shared_stats(idx) == want
    idx.release()


@pytest.mark.parametrize("case", ["unaligned", "d=500"])
@pytest.mark.gpu
def test_queries_that_would_be_copied_are_not_shared(torch_dev, case):
    """A query that pad_query has to copy (rows padded beyond d, or a pointer that is not 16-byte aligned) is staged in
    its search's context: such a search is not shared, and its results are the plain ones."""
    torch, dev = torch_dev
    d = 500 if case == "d=500" else 512
    idx = DeviceIndex(corpus(12_000, d), device=0)
    idx.set_variant(FORCE)
    st, feeder = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    m = SHARE_DEFAULT + 2
    q = unit_queries(m + 1, d, 61)
    if case == "unaligned":
        flat = torch.zeros((m + 1) * d + 1, device=dev, dtype=torch.float32)
        q_t = flat[1:].view(m + 1, d)
        q_t.copy_(torch.from_numpy(q))
        assert q_t[0].data_ptr() % 16 == 4 and q_t[1].data_ptr() % 16 == 4
    else:
        q_t = torch.from_numpy(q).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    assert [x for x in _native.last_launches() if x[0] != "gemv"][0][0].startswith("gemv_f16_oneshot_kernel<1,")
    same(got, (exp[0][1:], exp[1][1:]), case)
    assert shared_stats(idx) == {"shared_passes": 0, "claimed": 0, "empty_passes": 0}
    idx.release()


# ---- 5. isolation and life cycle --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_caller_streams_never_claim_each_other(torch_dev):
    torch, dev = torch_dev
    idx, st_a, feeder = make(torch, dev)
    st_b = torch.cuda.Stream(device=dev)
    m = 6
    q_t = torch.from_numpy(unit_queries(2 * m + 2, 512, 67)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st_a)
    warm_up(torch, dev, idx, q_t[1], 100, st_b)
    s, r = slots(torch, dev, 2 * m, 100)
    ev = sleeping_event(torch, dev, feeder)
    for i in range(2 * m):          # (even calls on a, odd calls on b; the first of each behind the event)
        call(idx, q_t[2 + i], 100, s[i], r[i], st_a if i % 2 == 0 else st_b, ready=ev if i < 2 else None)
    assert not ev.query()
    st_a.synchronize()
    st_b.synchronize()
    same(host(s, r), (exp[0][2:], exp[1][2:]))
    want = counters_of(claim_model(backlog_model(m), SHARE_DEFAULT))
    stats = idx.ahead_stats(shared=True)
    assert stats["pipelines"] == 2 and stats["plain"] == 0
    assert shared_stats(idx) == {k: 2 * v for k, v in want.items()}
    idx.release()


@pytest.mark.gpu
def test_tombstones_between_two_backlogs(torch_dev):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = SHARE_DEFAULT + 1
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 71)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    items = [(q_t[1 + i], 100) for i in range(m)]
    same(backlog(torch, dev, idx, items, st, feeder), (exp[0][1:], exp[1][1:]), "no tombstones")
    dead = sorted({int(x) for x in exp[1][:, :2].ravel()})
    idx.mask_rows(dead)
    exp2 = plain(torch, dev, idx, q_t, 100)
    assert not np.isin(exp2[1], dead).any()
    same(backlog(torch, dev, idx, items, st, feeder), (exp2[0][1:], exp2[1][1:]), "winners tombstoned")
    model = [S(0)] + [S(1, claimable=i > 0) for i in range(m)] + [S(2, claimable=i > 0) for i in range(m)]
    assert shared_stats(idx) == counters_of(claim_model(model, SHARE_DEFAULT))
    idx.release()


@pytest.mark.gpu
def test_append_past_the_capacity_between_backlogs(torch_dev):
    """The append drains the pipeline and moves the rows and the shadow: the second backlog starts a ring of its own."""
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = SHARE_DEFAULT + 1
    q = unit_queries(2 * m + 1, 512, 73)
    q_t = torch.from_numpy(q).to(dev)
    before = plain(torch, dev, idx, q_t[:m + 1], 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got1 = backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)
    extra = gaussian(3_000, 512, 74)
    extra[5:5 + m] = q[m + 1:]
    idx.append(extra)
    assert idx.n == 15_000
    # (the first call behind the append grows the ring's score vectors -- freeing the old ones waits for the device, the
    #  sleeping stream included -- so it is made here, on its own, and is search 0 of the new ring)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got2 = backlog(torch, dev, idx, [(q_t[m + 1 + i], 100) for i in range(m)], st, feeder)
    after = plain(torch, dev, idx, q_t[m + 1:], 100)
    assert after[1][:, 0].tolist() == [12_005 + i for i in range(m)]
    same(got1, (before[0][1:], before[1][1:]), "before the append")
    same(got2, after, "after the append")
    st1 = shared_stats(idx)
    assert st1["claimed"] == st1["empty_passes"] == 2 * (m - 1 - (m - 1) // SHARE_DEFAULT), st1
    idx.release()


@pytest.mark.gpu
def test_set_screen_between_backlogs(torch_dev):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = SHARE_DEFAULT + 1
    q_t = torch.from_numpy(unit_queries(3 * m + 1, 512, 79)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    got = [backlog(torch, dev, idx, [(q_t[1 + i], 100) for i in range(m)], st, feeder)]
    idx.set_screen(0)
    got.append(backlog(torch, dev, idx, [(q_t[1 + m + i], 100) for i in range(m)], st, feeder))
    assert _native.last_launches()[-1][0].startswith("gemv_f32_oneshot_kernel<")
    idx.set_screen(1)
    got.append(backlog(torch, dev, idx, [(q_t[1 + 2 * m + i], 100) for i in range(m)], st, feeder))
    assert _native.last_launches()[0][0].startswith("gemv_f16_oneshot_kernel<")
    for b in range(3):
        same(got[b], (exp[0][1 + b * m:1 + (b + 1) * m], exp[1][1 + b * m:1 + (b + 1) * m]), f"backlog {b}")
    model = ([S(0)] + [S(1, claimable=i > 0) for i in range(m)] + [S(2, share=False) for i in range(m)] +
             [S(3, claimable=i > 0) for i in range(m)])
    assert shared_stats(idx) == counters_of(claim_model(model, SHARE_DEFAULT))
    idx.release()


@pytest.mark.gpu
def test_release_with_a_backlog_enqueued(torch_dev):
    torch, dev = torch_dev
    idx, st, feeder = make(torch, dev)
    m = RING + 2
    q_t = torch.from_numpy(unit_queries(m + 1, 512, 83)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    warm_up(torch, dev, idx, q_t[0], 100, st)
    s, r = slots(torch, dev, m, 100)
    ev = sleeping_event(torch, dev, feeder)
    for i in range(m):
        call(idx, q_t[1 + i], 100, s[i], r[i], st, ready=ev if i == 0 else None)
    idx.release()                       # the only owner: the library drains what it enqueued
    torch.cuda.synchronize(dev)
    same(host(s, r), (exp[0][1:], exp[1][1:]))


# ---- 6. one mid-size case, no artificial backlog ----------------------------------------------------------------------
@pytest.mark.gpu
def test_mid_size_24_searches(torch_dev):
    """100,000 x 1536, screened by default, 24 searches back to back: how many passes are shared depends on how far the
    host gets ahead of the card, so only the results are checked (the counters are printed)."""
    torch, dev = torch_dev
    idx = DeviceIndex(corpus(100_000, 1536), device=0)
    st = torch.cuda.Stream(device=dev)
    q_t = torch.from_numpy(unit_queries(24, 1536, 89)).to(dev)
    exp = plain(torch, dev, idx, q_t, 100)
    s, r = slots(torch, dev, 24, 100)
    torch.cuda.synchronize(dev)
    for i in range(24):
        call(idx, q_t[i], 100, s[i], r[i], st)
    st.synchronize()
    same(host(s, r), exp)
    stats = shared_stats(idx)
    print("24 searches over 100,000 x 1536:", stats)
    assert stats["claimed"] == stats["empty_passes"]
    idx.release()

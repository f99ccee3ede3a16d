"""GPU: thin grids and the LDS-staged queries of the run-ahead pipeline's shared passes (svs_amd/csrc/pass_share.h,
gemv_f16.h; svs_index_search_device_ahead).

A search the host expects an earlier pass to serve launches its own pass on one resident set of workgroups; the kernel
walks all row blocks on any grid, so nothing depends on the guess.  svs_internal_tune(6, 2) makes EVERY shareable pass
thin (the working ones too), 1 none, 0 predicts.  Every case compares rows and uint32 score bits with the same queries
through svs_index_search_device -- the arithmetic is unchanged, so the difference allowed is zero -- and the claim
kernels' counters with the host model of tests/test_shared_pass_gpu.py, whose backlog (a first search behind a
sleeping ready event) is reused here.
"""
import functools

import numpy as np
import pytest

from svs_amd import DeviceIndex, _native
from test_shared_pass_gpu import (FORCE, RING, SHARE_DEFAULT, SHARE_MAX, SHARE_NSTEP_MAX, S, backlog, call, claim_model, counters_of,  # noqa: F401
                                  gaussian, host, plain, same, shared_stats, slots, torch_dev, unit_queries, warm_up)

SORT_CAP = 4096      # the window path (the only one whose searches share) starts above this many rows


def rows_per_block(d):
    """R * WPB of gemv_f16_oneshot_kernel<d / 512, R, WPB> (f16_rows_r / f16_rows_wpb in svs_amd.hip)."""
    nstep = d // 512
    r = 4 if nstep <= 1 else (2 if nstep <= 3 else 1)
    return r, r * (16 if nstep <= 6 else 8)


@functools.lru_cache(maxsize=2)
def corpus(d):
    """One matrix per row length, as long as the longest case needs (cases slice it); cases are ordered by d."""
    m = gaussian(66_000 if d == 512 else 33_000 if d <= 1536 else 25_000, d, 4000 + d)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def thin_grid(d):
    idx = DeviceIndex(corpus(d)[:1000], device=0)
    t = idx.ahead_stats(shared=True)["thin_grid"]
    idx.release()
    return t


@pytest.fixture
def thin_mode():
    """svs_internal_tune(6, v) during the test; the default (predict) afterwards."""
    lib = _native.load()

    def set_mode(v):
        assert lib.svs_internal_tune(6, v) == 0
    yield set_mode
    assert lib.svs_internal_tune(6, 0) == 0


def make(torch, dev, d, n, dtype):
    idx = DeviceIndex(corpus(d)[:n], device=0, dtype=dtype)
    idx.set_variant(FORCE if dtype == "f32" else 0)
    return idx, torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)


def thin_stats(idx):
    st = idx.ahead_stats(shared=True)
    return {k: st[k] for k in ("thin_passes", "thin_worked")}


def run_backlogs(torch, dev, idx, st, feeder, d, lengths, seed, k=100):
    """One warm-up call, then one backlog per length on the same pipeline; every result against the plain call.
    -> the model's searches (warm-up included)."""
    total = 1 + sum(lengths)
    q_t = torch.from_numpy(unit_queries(total, d, seed)).to(dev)
    exp = plain(torch, dev, idx, q_t, k)
    same(warm_up(torch, dev, idx, q_t[0], k, st), (exp[0][:1], exp[1][:1]), "warm-up")
    model, at = [S(0)], 1
    for b, m in enumerate(lengths):
        got = backlog(torch, dev, idx, [(q_t[at + i], k) for i in range(m)], st, feeder)
        same(got, (exp[0][at:at + m], exp[1][at:at + m]), f"backlog {b} of {m}")
        model += [S(1 + b, claimable=i > 0) for i in range(m)]
        at += m
    return model


# ---- 1. the thin grid does the work: every sharing geometry, one / two / three trips ---------------------------------
@pytest.mark.parametrize("trips", ["one-ragged", "two", "three-ragged"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", list(range(512, 512 * SHARE_NSTEP_MAX + 1, 512)))
@pytest.mark.gpu
def test_thin_grid_does_the_work(torch_dev, thin_mode, d, dtype, trips):
    torch, dev = torch_dev
    t, (_, rb) = thin_grid(d), rows_per_block(d)
    assert t > 0 and t % 256 == 0, t
    n = {"one-ragged": t * rb - 1, "two": t * rb + 1, "three-ragged": 2 * t * rb + rb + 1}[trips]
    assert n <= corpus(d).shape[0]
    thin_mode(2)
    idx, st, feeder = make(torch, dev, d, n, dtype)
    lengths = [1, SHARE_MAX, SHARE_MAX + 1]
    model = run_backlogs(torch, dev, idx, st, feeder, d, lengths, 7 + d)
    if n <= SORT_CAP:
        # One resident set of <6, 1, 16> is one workgroup per CU (its registers allow 7 waves per SIMD, a workgroup has
        # 16): 256 x 16 - 1 = 4095 rows take the sort path, whose searches never share.  Results as ever, nothing thin.
        assert (d, trips) == (3072, "one-ragged"), (d, trips, t, n)
        assert shared_stats(idx) == {"shared_passes": 0, "claimed": 0, "empty_passes": 0}
        assert thin_stats(idx) == {"thin_passes": 0, "thin_worked": 0}
        idx.release()
        return
    launches = [x for x in _native.last_launches() if x[0] != "gemv"]
    assert launches[0][0].startswith(f"gemv_f16_oneshot_kernel<{d // 512},") and launches[0][1:] == (n, 1), launches
    hist = claim_model(model, SHARE_DEFAULT)
    assert shared_stats(idx) == counters_of(hist), (d, dtype, n)
    # every pass was thin, and those that served anything worked on the thin grid
    assert thin_stats(idx) == {"thin_passes": len(model), "thin_worked": sum(hist[1:])}, (d, dtype, n)
    assert idx.ahead_stats(shared=True)["thin_grid"] == t
    idx.release()


# ---- 2. the tail workgroup of the LDS fill: waves without rows take part and leave behind the barrier ---------------
@pytest.mark.parametrize("tail", ["one-wave", "one-row"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("d", [512, 1536, 3072, 3584])
@pytest.mark.gpu
def test_lds_fill_in_the_tail_workgroup(torch_dev, d, dtype, tail):
    torch, dev = torch_dev
    r, rb = rows_per_block(d)
    blocks = -(-(SORT_CAP + 100) // rb)
    n = blocks * rb + (r if tail == "one-wave" else 1)
    idx, st, feeder = make(torch, dev, d, n, dtype)
    lengths = list(range(1, SHARE_MAX + 1))          # the first search of a backlog of c serves all c
    model = run_backlogs(torch, dev, idx, st, feeder, d, lengths, 11 + d)
    hist = claim_model(model, SHARE_DEFAULT)
    assert hist[1:] == [2] + [1] * (SHARE_MAX - 1), hist     # (c = 1: the warm-up and the backlog of one)
    assert shared_stats(idx) == counters_of(hist)
    assert thin_stats(idx) == {"thin_passes": hist[0], "thin_worked": 0}
    idx.release()


# ---- 3. prediction on a blocked pipeline: thin exactly where the model's passes are empty ----------------------------
@pytest.mark.parametrize("case", ["2", "4", "5", "2R+3", "timed", "event"])
@pytest.mark.gpu
def test_prediction_on_a_blocked_pipeline(torch_dev, case):
    torch, dev = torch_dev
    d, k = 512, 100
    idx, st, feeder = make(torch, dev, d, 12_000, "f32")
    m = {"2": 2, "4": 4, "5": 5, "2R+3": 2 * RING + 3, "timed": 2 * RING + 1, "event": 7}[case]
    q_t = torch.from_numpy(unit_queries(m + 1, d, 17 + m)).to(dev)
    exp = plain(torch, dev, idx, q_t, k)
    warm_up(torch, dev, idx, q_t[0], k, st)
    items = [(q_t[1 + i], k) for i in range(m)]
    if case == "timed":                      # (the step counter starts over: backlog searches 0, 4, 8, ... are timed)
        idx.set_timing(4)
        got = backlog(torch, dev, idx, items, st, feeder)
        idx.get_timing()
        idx.set_timing(0)
        model = [S(0)] + [S(1, claimable=(i > 0 and i % 4 != 0)) for i in range(m)]
    elif case == "event":
        got = backlog(torch, dev, idx, items, st, feeder, events={2})
        model = [S(0)] + [S(1, claimable=i not in (0, 2)) for i in range(m)]
    else:
        got = backlog(torch, dev, idx, items, st, feeder)
        model = [S(0)] + [S(1, claimable=i > 0) for i in range(m)]
    same(got, (exp[0][1:], exp[1][1:]), case)
    hist = claim_model(model, SHARE_DEFAULT)
    assert hist[0] > 0
    assert shared_stats(idx) == counters_of(hist)
    assert thin_stats(idx) == {"thin_passes": hist[0], "thin_worked": 0}, case
    idx.release()


# ---- 4. a caller that never queues: no thin pass, every pass serves its own search -----------------------------------
@pytest.mark.gpu
def test_never_queuing_caller(torch_dev):
    torch, dev = torch_dev
    d, k, m = 512, 100, 12
    idx, st, _ = make(torch, dev, d, 12_000, "f32")
    q_t = torch.from_numpy(unit_queries(m, d, 23)).to(dev)
    exp = plain(torch, dev, idx, q_t, k)
    s, r = slots(torch, dev, m, k)
    for i in range(m):
        call(idx, q_t[i], k, s[i], r[i], st)
        st.synchronize()
    same(host(s, r), exp)
    assert shared_stats(idx) == {"shared_passes": 0, "claimed": 0, "empty_passes": 0}
    assert thin_stats(idx) == {"thin_passes": 0, "thin_worked": 0}
    idx.release()


# ---- 5. a model that disagrees with the device heals at the next search nothing can claim ---------------------------
@pytest.mark.gpu
def test_divergence_heals(torch_dev, thin_mode):
    torch, dev = torch_dev
    d, k, m = 512, 100, 2 * SHARE_MAX + 1
    idx, st, feeder = make(torch, dev, d, 12_000, "f32")
    q_t = torch.from_numpy(unit_queries(2 * m + 1, d, 29)).to(dev)
    exp = plain(torch, dev, idx, q_t, k)
    thin_mode(2)
    warm_up(torch, dev, idx, q_t[0], k, st)
    got1 = backlog(torch, dev, idx, [(q_t[1 + i], k) for i in range(m)], st, feeder)
    first = thin_stats(idx)
    assert first["thin_passes"] == m + 1 and first["thin_worked"] > 0
    thin_mode(0)
    got2 = backlog(torch, dev, idx, [(q_t[1 + m + i], k) for i in range(m)], st, feeder)
    same(got1, (exp[0][1:1 + m], exp[1][1:1 + m]), "every pass thin")
    same(got2, (exp[0][1 + m:], exp[1][1 + m:]), "predicted")
    model = [S(0)] + [S(1, claimable=i > 0) for i in range(m)] + [S(2, claimable=i > 0) for i in range(m)]
    hist = claim_model(model, SHARE_DEFAULT)
    second = thin_stats(idx)
    assert shared_stats(idx) == counters_of(hist)
    assert second["thin_worked"] == first["thin_worked"], (first, second)
    assert second["thin_passes"] - first["thin_passes"] == hist[0] - claim_model(model[:1 + m], SHARE_DEFAULT)[0] > 0
    idx.release()


# ---- 6. mode 1: the one-shot grid for every pass ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.gpu
def test_mode_one_never_launches_a_thin_grid(torch_dev, thin_mode, dtype):
    torch, dev = torch_dev
    d, n = 1536, 12_001
    thin_mode(1)
    idx, st, feeder = make(torch, dev, d, n, dtype)
    model = run_backlogs(torch, dev, idx, st, feeder, d, [SHARE_MAX + 2, 2 * RING + 3], 31)
    launches = [x for x in _native.last_launches() if x[0] != "gemv"]
    assert launches[0][0].startswith("gemv_f16_oneshot_kernel<3, 2, 16>") and launches[0][1:] == (n, 1), launches
    hist = claim_model(model, SHARE_DEFAULT)
    assert hist[0] > 0 and shared_stats(idx) == counters_of(hist)
    assert thin_stats(idx) == {"thin_passes": 0, "thin_worked": 0}
    idx.release()

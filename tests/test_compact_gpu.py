"""GPU: svs_index_compact -- tombstoned rows removed in place in HBM (svs_amd/csrc/compact.h).

The compacted index must BE the index a rebuild from the live rows gives: the row map is the live rows ascending,
what is stored moved bit for bit (fp8 scales and the f32 index's half shadow with their rows), and every search entry
returns the same rows and the same score bits as a fresh index of the live rows of the source matrix.  The cases run
through svs_internal_compact with bounce buffers of 1 row, 64 rows and the default, so that DIRECT steps, BOUNCE steps
and their mixtures all move rows; the step counts the call reports must be those of the host planner."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from svs_amd import DeviceIndex, _native

N = 5000
GEOMETRIES = [("f32", 3), ("f32", 24), ("f32", 1536), ("f32", 4100), ("f16", 24), ("f16", 1536), ("fp8", 24), ("fp8", 3072)]
ELEM = {"f32": 4, "f16": 2, "fp8": 1}


def _random_quarter(n):
    return np.sort(np.random.default_rng(5).choice(n, n // 4, replace=False))


PATTERNS = {
    "none": lambda n: np.array([], dtype=np.int64),
    "row0": lambda n: np.array([0]),
    "last": lambda n: np.array([n - 1]),
    "alternate": lambda n: np.arange(0, n, 2),
    "first_half": lambda n: np.arange(n // 2),
    "all_but_last": lambda n: np.arange(n - 1),
    "all": lambda n: np.arange(n),
    "random_quarter": _random_quarter,
}
BOUNCES = (1, 64, 0)   # 0: the default, about 32 MiB of rows


@functools.lru_cache(maxsize=None)
def source(d):
    m = np.random.default_rng(1000 + d).standard_normal((N, d)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


@functools.lru_cache(maxsize=None)
def queries(d):
    q = np.random.default_rng(2000 + d).standard_normal((64, d)).astype(np.float32)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def answers(idx, d, n_live):
    """Everything a caller can ask of the index, as comparable arrays."""
    q = queries(d)
    if n_live == 0:
        with pytest.raises(ValueError):
            idx.search_batch(q[:1], 10)
        return {"pairs": idx.top_pairs(10)}
    out = {}
    for name, qq, k in (("q1", q[:1], 10), ("q1_all", q[1:2], N + 7), ("q16", q[:16], 10), ("q64", q, 25)):
        s, r = idx.search_batch(qq, k)
        assert s.shape[1] == min(k, n_live), (name, s.shape, n_live)      # count = min(k, n)
        out[name] = (bits(s), r)
    rows = np.arange(0, n_live, 3)[::-1] + idx.row_offset
    if idx.ld * ELEM[idx.dtype] <= 16384:
        s, r = idx.search_batch_within(q[:3], 10, rows)
        out["within"] = (bits(s), r)
    else:                                      # svs_index_search_rows takes rows of up to 16 KiB, compacted or not
        with pytest.raises(NotImplementedError):
            idx.search_batch_within(q[:3], 10, rows)
    out["scores"] = bits(idx.scores(q[5]))
    out["pairs"] = idx.top_pairs(20)
    return out


def same(a, b, label):
    assert a.keys() == b.keys()
    for key in a:
        if key == "pairs":
            assert [(np.float32(s).view(np.uint32), i, j) for s, i, j in a[key]] == \
                   [(np.float32(s).view(np.uint32), i, j) for s, i, j in b[key]], (label, key)
        elif key == "scores":
            assert np.array_equal(a[key], b[key]), (label, key)
        else:
            assert np.array_equal(a[key][1], b[key][1]), (label, key, "rows")
            assert np.array_equal(a[key][0], b[key][0]), (label, key, "score bits")


def planned(dead, n, bounce_rows):
    lib = _native.load()
    dead = np.ascontiguousarray(dead, dtype=np.uint32)
    total = int(lib.svs_internal_compact_plan(dead.ctypes.data, len(dead), n, bounce_rows, None, 0))
    steps = np.zeros((max(total, 1), 3), dtype=np.int64)
    assert lib.svs_internal_compact_plan(dead.ctypes.data, len(dead), n, bounce_rows, steps.ctypes.data, total) == total
    return steps[:total]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("dtype,d", GEOMETRIES, ids=[f"{t}-{d}" for t, d in GEOMETRIES])
def test_compacted_index_is_the_rebuilt_index(gpu, dtype, d, pattern):
    m = source(d)
    dead = PATTERNS[pattern](N)
    live = np.setdiff1d(np.arange(N), dead)
    off = 70_000
    fresh = DeviceIndex(m[live], device=0, dtype=dtype, row_offset=off)
    want = answers(fresh, d, len(live))
    want_rows = fresh.stored_rows()
    fresh.release()
    kinds = {}
    for bounce in BOUNCES:
        label = f"{dtype} d={d} {pattern} bounce={bounce}"
        idx = DeviceIndex(m, device=0, dtype=dtype, row_offset=off)
        before = idx.stored_rows()
        hbm = idx.hbm_bytes
        if len(dead):
            idx.mask_rows(dead[::-1] + off)            # (any order: the library sorts)
        assert idx.n_masked == len(dead)
        stats = []
        row_map = idx.compact(bounce_rows=bounce, stats=stats)
        assert np.array_equal(row_map, live + off), label
        assert (idx.n, idx.n_masked, idx.hbm_bytes) == (len(live), 0, hbm), label
        after = idx.stored_rows()
        assert np.array_equal(bits(after), bits(before[live])), label        # (fp8: the scales moved with their rows)
        assert np.array_equal(bits(after), bits(want_rows)), label
        # what the call says it did is the host plan for this bounce size
        row_b = idx.ld * ELEM[dtype]
        per_row = row_b + (4 if dtype == "fp8" else 0) + (idx.ld * 2 if idx.screen_stats()["shadow"] == 1 else 0)
        steps = planned(dead, N, bounce if bounce else max(1, (32 << 20) // row_b))
        n_direct, n_bounce = int((steps[:, 0] == 0).sum()), int((steps[:, 0] == 1).sum())
        moved = int(steps[:, 2].sum())
        assert stats == [n_direct, n_bounce, moved, moved * per_row], (label, stats)
        first_dead = int(dead[0]) if len(dead) else N
        assert moved == max(len(live) - first_dead, 0), label
        kinds[bounce] = (n_direct, n_bounce)
        same(answers(idx, d, len(live)), want, label)
        idx.release()
    if pattern == "random_quarter":
        assert kinds[1][0] > 0 and kinds[1][1] == 0                      # one row of bounce buffer: the gap always suffices
        assert kinds[64][0] > 0 and kinds[64][1] > 0                      # both kinds in one compaction
        assert kinds[0][0] == 0 and kinds[0][1] in (1, 2)                 # the default buffer takes the rest in one or two steps
    if pattern == "row0":
        assert kinds[64] == (0, -(-(N - 1) // 64)) and kinds[1] == (N - 1, 0)
    if pattern == "alternate":
        assert kinds[64][0] > 0 and kinds[64][1] > 0
    if pattern == "first_half":
        assert kinds[1] == kinds[64] == (1, 0)
    if pattern in ("none", "last", "all"):
        assert set(kinds.values()) == {(0, 0)}                            # nothing to move


@pytest.mark.gpu
def test_rows_longer_than_16_kib_were_among_the_cases(gpu):
    idx = DeviceIndex(source(4100)[:8], device=0)
    assert idx.ld * 4 > 16384
    idx.release()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 8192])
def test_f32_index_with_a_shadow_after_compaction(gpu, n):
    """An f32 index with its half shadow, d = 512, under set_variant(12) (screen whatever the row count): the shadow rows
    must have moved with the f32 rows.  A single query is screened only on the window path of the selection stage, i.e.
    with more than SORT_CAP = 4,096 rows (plan_search), so at n = 4,096 -- 3,072 rows after the compaction -- neither
    the compacted nor the fresh index can screen, and the check there is that both launch the same kernels and agree;
    at n = 8,192 (6,144 rows left) the search IS screened, reads the moved shadow, and screen_stats must say so.  Then
    100 rows are appended (the tail of the buffers serves them), 3 masked, and the search repeated."""
    d, k = 512, 50
    rng = np.random.default_rng(41)
    m = rng.standard_normal((n, d)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    extra = rng.standard_normal((100, d)).astype(np.float32)
    extra /= np.linalg.norm(extra, axis=1, keepdims=True)
    q = m[77] + 0.3 * rng.standard_normal(d).astype(np.float32)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    dead = np.sort(rng.choice(n, n // 4, replace=False))
    live = np.setdiff1d(np.arange(n), dead)

    def search(idx):
        before = idx.screen_stats()
        s, r = idx.search_batch(q[None, :], k)
        names = [x[0] for x in _native.last_launches()]
        after = idx.screen_stats()
        assert after["shadow"] == 1 and not after["paused"]
        if idx.n > 4096:
            assert names[0].startswith("gemv_f16_oneshot_kernel<") and names[1].startswith("rescore_f32_kernel<"), names
            assert after["screened"] + after["fallback"] - before["screened"] - before["fallback"] == 1
        return bits(s), r, names

    fresh = DeviceIndex(m[live], device=0)
    fresh.set_variant(12)
    idx = DeviceIndex(m, device=0)
    idx.set_variant(12)
    assert idx.screen_stats()["shadow"] == 1 and idx.hbm_bytes == n * d * 6
    idx.mask_rows(dead)
    stats = []
    assert np.array_equal(idx.compact(bounce_rows=64, stats=stats), live)
    assert stats[0] > 0 and stats[1] > 0 and stats[3] == stats[2] * d * 6     # the shadow rows went along
    a, b = search(idx), search(fresh)
    assert a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    # the tail of the buffers serves later appends; tombstones start over
    for i in (idx, fresh):
        i.append(extra)
        i.mask_rows([5, len(live) - 1, len(live) + 50])
        assert (i.n, i.n_masked) == (len(live) + 100, 3)
    a, b = search(idx), search(fresh)
    assert a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    s, r = idx.search_batch(extra[50:51], 5)
    assert len(live) + 50 not in r[0]
    idx.release(); fresh.release()


@pytest.mark.gpu
def test_compaction_while_a_thread_searches(gpu):
    """Every answer is a valid answer of one of the two numberings; no error; the final state is the fresh index."""
    n, d, k = 20_000, 256, 10
    rng = np.random.default_rng(51)
    m = rng.standard_normal((n, d)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    qs = rng.standard_normal((4, d)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    dead = np.sort(rng.choice(n, n // 4, replace=False))
    live = np.setdiff1d(np.arange(n), dead)
    m64, q64 = m.astype(np.float64), qs.astype(np.float64)
    idx = DeviceIndex(m, device=0)
    other = idx.share()
    got, errors, stop = [], [], threading.Event()

    def loop():
        try:
            j = 0
            while not stop.is_set():
                got.append((j % 4, other.search(qs[j % 4], k)))
                j += 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=loop)
    t.start()
    try:
        while len(got) < 4 and not errors:
            pass
        idx.mask_rows(dead)
        row_map = idx.compact()
        mark = len(got)                                       # (a search in flight now may still have run before the call)
        while len(got) < mark + 2 and not errors and t.is_alive():
            pass
    finally:
        stop.set()
        t.join(60)
    assert not errors, errors
    assert np.array_equal(row_map, live)
    # a score is the f32 dot product of 256 unit-norm terms: within 1e-5 of the f64 one (the bound the smoke test uses)
    tol, fits = 1e-5, {"old": 0, "new": 0}
    for j, res in got:
        assert len(res) == k
        rows = np.array([r for _, r in res])
        sc = np.array([s for s, _ in res])
        err_old = np.abs(m64[rows] @ q64[j] - sc).max()
        err_new = np.abs(m64[live[rows]] @ q64[j] - sc).max() if rows.max() < len(live) else np.inf
        assert min(err_old, err_new) <= tol, (j, res, err_old, err_new)
        fits["old" if err_old <= err_new else "new"] += 1
    print(f"{len(got)} searches beside the compaction: {fits}")
    assert fits["old"] > 0 and fits["new"] > 0
    fresh = DeviceIndex(m[live], device=0)
    for j in range(4):
        a, b = idx.search_batch(qs[j:j + 1], k), fresh.search_batch(qs[j:j + 1], k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    other.release(); idx.release(); fresh.release()


@pytest.mark.gpu
def test_run_ahead_searches_enqueued_before_the_call_keep_the_old_numbering(gpu):
    import torch
    n, d, k = 6000, 1536, 20
    rng = np.random.default_rng(61)
    m = rng.standard_normal((n, d)).astype(np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    dead = np.sort(rng.choice(n, n // 4, replace=False))
    live = np.setdiff1d(np.arange(n), dead)
    g = torch.Generator(device="cuda")
    g.manual_seed(62)
    qs = torch.randn((12, d), device="cuda", generator=g)
    qs /= qs.norm(dim=1, keepdim=True)
    st = torch.cuda.current_stream().cuda_stream

    def run(idx, js, ahead):
        out_s = torch.full((12, k), -1.0, device="cuda")
        out_r = torch.full((12, k), -1, device="cuda", dtype=torch.int64)
        for j in js:
            (idx.search_device_ahead if ahead else idx.search_device)(qs[j].data_ptr(), 1, d, k, out_s[j].data_ptr(),
                                                                      out_r[j].data_ptr(), stream=st)
        return out_s, out_r

    torch.cuda.synchronize()
    masked = DeviceIndex(m, device=0, dtype="f16")
    masked.mask_rows(dead)
    fresh = DeviceIndex(m[live], device=0, dtype="f16")
    want_old = run(masked, range(8), False)
    want_new = run(fresh, range(8, 12), False)
    idx = DeviceIndex(m, device=0, dtype="f16")
    idx.mask_rows(dead)
    got_s, got_r = run(idx, range(8), True)                  # enqueued, not waited for
    row_map = idx.compact(bounce_rows=64)
    out_s = torch.full((12, k), -1.0, device="cuda")
    out_r = torch.full((12, k), -1, device="cuda", dtype=torch.int64)
    for j in range(8, 12):
        idx.search_device_ahead(qs[j].data_ptr(), 1, d, k, out_s[j].data_ptr(), out_r[j].data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(row_map, live)
    assert idx.ahead_stats()["ahead"] == 12
    assert torch.equal(got_r[:8], want_old[1][:8]) and torch.equal(got_s[:8].view(torch.int32), want_old[0][:8].view(torch.int32))
    assert torch.equal(out_r[8:], want_new[1][8:]) and torch.equal(out_s[8:].view(torch.int32), want_new[0][8:].view(torch.int32))
    assert int(out_r[8:].max()) < len(live)
    # old row of a result enqueued before the call, through the map, is what the same search finds afterwards
    s2, r2 = idx.search_batch(qs[:1].cpu().numpy(), k)
    assert np.array_equal(row_map[r2[0]], got_r[0].cpu().numpy())
    for i in (idx, masked, fresh):
        i.release()


@pytest.mark.gpu
def test_byte_offsets_past_4_gib(gpu):
    """An f16 index just past 2^32 bytes, built from device blocks: rows far above the 4 GiB offset move to
    destinations on both sides of it."""
    import torch
    d, block, nblocks = 1536, 71_000, 22
    n = block * nblocks
    assert n * d * 2 > (1 << 32) + (100 << 20)

    def make(b):
        g = torch.Generator(device="cuda")
        g.manual_seed(7000 + b)
        return torch.randn((block, d), device="cuda", generator=g)

    idx = DeviceIndex.empty(d, device=0, dtype="f16", reserve=n)
    for b in range(nblocks):
        t = make(b)
        idx.append_device(t.data_ptr(), block)
        del t
    assert idx.n == n and idx.hbm_bytes == n * d * 2
    dead = np.arange(3, n, 10)                                # a tenth of the rows, up to the last block's last rows
    assert dead[-1] > n - 10
    live = np.setdiff1d(np.arange(n), dead)
    idx.mask_rows(dead)
    stats = []
    row_map = idx.compact(stats=stats)
    assert np.array_equal(row_map, live) and idx.n == len(live) and idx.n_masked == 0
    assert stats[0] > 0 and stats[2] == len(live) - 3 and stats[3] == stats[2] * d * 2
    edge = (1 << 32) // (d * 2)                               # the row the 4 GiB offset falls into
    assert edge + 500 < len(live) - 1000
    for row0 in (len(live) - 1000, edge - 500):
        got = idx.stored_rows(row0, 1000)
        old = live[row0:row0 + 1000]
        want = np.empty_like(got)
        for b in np.unique(old // block):
            t = make(int(b))
            sel = old // block == b
            want[sel] = t[torch.from_numpy(old[sel] % block).cuda()].half().float().cpu().numpy()
            del t
        assert np.array_equal(bits(got), bits(want)), row0
    idx.release()


@pytest.mark.gpu
def test_c_abi_capacity_and_null_map(gpu):
    lib = _native.load()
    m = source(24)
    idx = DeviceIndex(m, device=0)
    dead = np.arange(10, 2000, 2)
    idx.mask_rows(dead)
    live = N - len(dead)
    q = queries(24)[:1]
    s0, r0 = idx.search_batch(q, 10)
    small = np.full(live, -1, dtype=np.int64)
    out_n = C.c_int64(-1)
    rc = lib.svs_index_compact(idx._handle(), small.ctypes.data, live - 1, C.byref(out_n))
    assert rc == _native.SVS_ERR_INVALID and out_n.value == live and (small == -1).all()
    idx._refresh()
    assert (idx.n, idx.n_masked) == (N, len(dead))
    s1, r1 = idx.search_batch(q, 10)
    assert np.array_equal(r0, r1) and np.array_equal(bits(s0), bits(s1))       # nothing changed
    out_n = C.c_int64(-1)
    assert lib.svs_index_compact(idx._handle(), None, 0, C.byref(out_n)) == _native.SVS_OK and out_n.value == live
    idx._refresh()
    assert (idx.n, idx.n_masked) == (live, 0)
    assert lib.svs_index_compact(idx._handle(), None, 0, None) == _native.SVS_OK       # no tombstones: nothing to do
    ident = idx.compact()
    assert np.array_equal(ident, np.arange(live))
    fresh = DeviceIndex(m[np.setdiff1d(np.arange(N), dead)], device=0)
    s2, r2 = idx.search_batch(q, 10)
    s3, r3 = fresh.search_batch(q, 10)
    assert np.array_equal(r2, r3) and np.array_equal(bits(s2), bits(s3))
    assert lib.svs_index_compact(None, None, 0, None) == _native.SVS_ERR_INVALID
    idx.release(); fresh.release()
    with pytest.raises(RuntimeError):
        idx.compact()


@pytest.mark.gpu
def test_kb_deletes_past_the_threshold_compact_the_hbm_copy(gpu, tmp_path):
    import svs_amd
    n, d = 400, 64
    vecs = np.random.default_rng(71).standard_normal((n + 10, d))
    vecs /= np.linalg.norm(vecs, axis=1, keepdims=True)
    table = {f"doc {i}": [float(x) for x in vecs[i]] for i in range(n + 10)}

    async def ef(texts):
        return [table[t] for t in texts]

    path = str(tmp_path / "kb.sqlite")
    kb = svs_amd.KB(path, ef)
    with kb.bulk_add_docs() as add_doc:
        for i in range(n):
            add_doc(f"doc {i}")
    kb.load()
    first = kb.embeddings_matrix.index
    with kb.bulk_del_docs() as del_doc:
        for i in range(100, 220):
            del_doc(i + 1)
    assert kb.embeddings_matrix.index is first and (first.n, first.n_masked) == (n - 120, 0)
    with kb.bulk_add_docs() as add_doc:
        add_doc(f"doc {n}")
    fresh = svs_amd.KB(path, ef)
    ids = lambda res: [(r["doc"]["id"], r["score"]) for r in res]
    for q in ("doc 5", "doc 150", "doc 399", f"doc {n}", f"doc {n + 3}"):
        assert ids(kb.retrieve(q, 12)) == ids(fresh.retrieve(q, 12)), q
    docs = [i + 1 for i in range(0, 100, 3)] + [i + 1 for i in range(220, 400, 7)]
    assert ids(kb.retrieve_within("doc 7", 9, docs)) == ids(fresh.retrieve_within("doc 7", 9, docs))
    assert [ids(r) for r in kb.retrieve_many(["doc 1", "doc 300"], 5)] == [ids(r) for r in fresh.retrieve_many(["doc 1", "doc 300"], 5)]
    assert [(s, a["id"], b["id"]) for s, a, b in kb.document_top_pairwise_scores(10)] == \
           [(s, a["id"], b["id"]) for s, a, b in fresh.document_top_pairwise_scores(10)]
    assert len(kb.retrieve("doc 1", 1000)) == n - 120 + 1
    kb.close(); fresh.close()

"""GPU: size-independent properties at BASELINE.json's full sizes, where the numpy
oracle would take minutes per query (the oracle-checked cases at these sizes are the
golden 1M x 1536 single-query vectors in test_search_gpu.py).

  * batch == loop: a batched search is by definition the per-query searches in order
    (the reference loops np.dot, src/svs/kb.py:1623);
  * fused == materialised: the fused top-k epilogue (no score matrix) must return exactly
    what the same kernel returns when every score is written and selected from
    (svs_index_set_variant(6) turns the fusion off) -- bit for bit, same summation order;
  * a planted row is found: a corpus row equal to the query scores 1 and comes first.

Corpora are generated on the device (torch is plumbing here: device memory and RNG)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _corpus(n, d, seed, block=250_000):
    import torch
    dev = torch.device("cuda:0")
    out = torch.empty((n, d), device=dev, dtype=torch.float32)
    for b0 in range(0, n, block):
        g = torch.Generator(device=dev)
        g.manual_seed(seed * 1_000_003 + b0)
        x = torch.randn((min(block, n - b0), d), device=dev, dtype=torch.float32, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        out[b0:b0 + x.shape[0]] = x
        del x
    return out


def _queries(nq, d, seed):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    q = torch.randn((nq, d), device="cuda:0", dtype=torch.float32, generator=g)
    q /= q.norm(dim=1, keepdim=True)
    return q


def _index(rows, dtype):
    import torch
    from svs_amd import DeviceIndex
    idx = DeviceIndex.from_device_pointer(rows.data_ptr(), rows.shape[0], rows.shape[1], device=0, dtype=dtype)
    torch.cuda.synchronize()
    return idx


def _same_up_to_near_ties(s_a, r_a, s_b, r_b, tol):
    """Two exact top-k lists computed in different summation orders: scores agree within
    tol, and rows agree wherever the neighbouring scores are further apart than tol."""
    assert np.max(np.abs(s_a - s_b)) <= tol
    diff = np.nonzero(r_a != r_b)[0]
    for i in diff:
        lo, hi = max(0, i - 1), min(len(s_a) - 1, i + 1)
        assert min(abs(s_a[i] - s_a[lo]) if lo != i else 1.0, abs(s_a[i] - s_a[hi]) if hi != i else 1.0) <= 2 * tol, \
            f"rank {i}: rows {r_a[i]} vs {r_b[i]} differ without a near tie"


def test_config1_f32_batch16_equals_single_queries(gpu):
    """BASELINE configs[1] size (1M x 1536 f32): 16 queries per corpus pass (4x4x1 MFMA kernel,
    fused top-k) against 16 single-query searches (GEMV + materialised top-k)."""
    import torch
    n, d, k = 1_000_000, 1536, 100
    rows = _corpus(n, d, 4242)
    qs = _queries(16, d, 99)
    planted = 777_777
    qs[3] = rows[planted]
    idx = _index(rows, "f32")
    del rows
    torch.cuda.empty_cache()
    qh = qs.cpu().numpy()
    bs, br = idx.search_batch(qh, k)
    assert bs.shape == (16, k)
    for qi in range(16):
        one = idx.search(qh[qi], k)
        s1 = np.array([s for s, _ in one], dtype=np.float32)
        r1 = np.array([r for _, r in one], dtype=np.int64)
        _same_up_to_near_ties(bs[qi], br[qi], s1, r1, 2e-6)
        assert np.all(np.diff(bs[qi]) <= 0)
    assert br[3, 0] == planted and abs(bs[3, 0] - 1.0) < 1e-5
    # and the fused epilogue loses nothing: materialised run of the same kernel, bit for bit
    idx.set_variant(6)
    ms, mr = idx.search_batch(qh, k)
    assert np.array_equal(mr, br) and np.array_equal(ms, bs)
    idx.release()


def test_config2_f16_b1024_fused_equals_materialised(gpu):
    """BASELINE configs[2]: 1M x 1536 f16, 1024 queries per call.  The fused run never writes
    the 4 GB score matrix; the materialised run of the same GEMM does, 256 queries at a time.
    Queries equal to rows 123,456, n - 1 (the last, partial row tile) and 0 come first in their lists, and queries
    of every query tile are checked against the oracle on the stored corpus."""
    import torch
    from svs_amd import _native
    from compare import assert_topk_parity
    from oracle import svs_oracle as oracle
    n, d, k, nq = 1_000_000, 1536, 100, 1024
    rows = _corpus(n, d, 5151)
    qs = _queries(nq, d, 17)
    planted = {1000: 123_456, 1001: n - 1, 1002: 0}
    for qi, row in planted.items():
        qs[qi] = rows[row]
    idx = _index(rows, "f16")
    del rows
    torch.cuda.empty_cache()
    qh = qs.cpu().numpy()
    fs, fr = idx.search_batch(qh, k)
    launches = _native.last_launches()
    assert [x[0] for x in launches if x[1] == n][:1] == ["gemm_phased_kernel<true, 2, 0, 256>"], launches
    for qi, row in planted.items():
        assert fr[qi, 0] == row and abs(fs[qi, 0] - 1.0) < 2e-3, (qi, row, fr[qi, :3])   # f16 rounding of a unit vector
    assert np.all(np.diff(fs, axis=1) <= 0) and fr.min() >= 0 and fr.max() < n
    idx.set_variant(6)
    for q0 in range(0, nq, 256):
        ms, mr = idx.search_batch(qh[q0:q0 + 256], k)
        assert np.array_equal(mr, fr[q0:q0 + 256]) and np.array_equal(ms, fs[q0:q0 + 256]), f"queries {q0}.."
    # a single-query search (GEMV kernel, other summation order) agrees up to near ties
    idx.set_variant(0)
    for qi in (0, 511, 1000, 1023):
        one = idx.search(qh[qi], k)
        _same_up_to_near_ties(fs[qi], fr[qi], np.array([s for s, _ in one], dtype=np.float32),
                              np.array([r for _, r in one], dtype=np.int64), 4e-6)
    # the oracle on the stored corpus (6 GB of f32 on the host), f64 truth computed in row blocks
    check = [0, 255, 256, 511, 1000, 1001, 1002, 1023]
    md = idx.stored_rows()
    idx_q = [idx.stored_query(qh[qi]) for qi in check]
    idx.release()
    q64 = np.array(idx_q, dtype=np.float64).T
    truth = np.empty((len(check), n))
    for r0 in range(0, n, 65536):
        truth[:, r0:r0 + 65536] = (md[r0:r0 + 65536].astype(np.float64) @ q64).T
    for j, qi in enumerate(check):
        exp = oracle.cpu_search(md, idx_q[j], k)
        assert_topk_parity(fs[qi], fr[qi], [x for x, _ in exp], [i for _, i in exp], truth[j], label=f"configs[2] q{qi}")
    del md


def _build_in_blocks(n, d, dtype, seed, planted, block=500_000, row_offset=0):
    """An index of n rows built block by block on the device (svs_index_reserve +
    svs_index_append_from_device): the f32 source of the whole corpus -- 77 GB for configs[3]'s
    shard, 123 GB for configs[4] -- never exists; one 500k-row block at a time does.
    `planted`: {row: query tensor} rows overwritten with given unit vectors."""
    import torch
    from svs_amd import DeviceIndex
    idx = DeviceIndex.empty(d, dtype=dtype, reserve=n, row_offset=row_offset)
    dev = torch.device("cuda:0")
    for b0 in range(0, n, block):
        rows = min(block, n - b0)
        g = torch.Generator(device=dev)
        g.manual_seed(seed * 1_000_003 + b0)
        x = torch.randn((rows, d), device=dev, dtype=torch.float32, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        for r, v in planted.items():
            if b0 <= r < b0 + rows:
                x[r - b0] = v
        torch.cuda.synchronize()
        idx.append_device(x.data_ptr(), rows)
        del x
    torch.cuda.empty_cache()
    assert idx.shape == (n, d)
    return idx


def _block_rows(n, d, seed, r0, r1, block=500_000):
    """Rows [r0, r1) of the corpus _build_in_blocks generates (regenerated, f32, on the host)."""
    import torch
    dev = torch.device("cuda:0")
    out = []
    for b0 in range(r0 // block * block, r1, block):
        rows = min(block, n - b0)
        g = torch.Generator(device=dev)
        g.manual_seed(seed * 1_000_003 + b0)
        x = torch.randn((rows, d), device=dev, dtype=torch.float32, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        out.append(x[max(r0, b0) - b0:min(r1, b0 + rows) - b0].cpu().numpy())
        del x
    return np.concatenate(out)


def test_config3_shard_f16_12p5m_rows(gpu):
    """BASELINE configs[3]: 100M x 1536 f16 row-sharded over 8 GPUs -- the PER-GPU shard at its
    stated size, 12.5M x 1536 halves = 1.92e10 elements (past 2^31 and 2^32 element offsets,
    38.4 GB) as ONE index on one card, with the shard's row_offset (rank 7 of 8).
      * planted rows near row 0, on both sides of element offset 2^31 and 2^32, and in the last
        tile are found first, with GLOBAL row numbers (64-bit addressing of every f16 kernel);
      * batch-16 (streaming MFMA kernel, fused top-k) == the 16 single-query searches up to near
        ties; batch-64 (tiled kernel) likewise on a sample;
      * the returned rows' scores, recomputed on the host from the regenerated rows, match
        (SURVEY section 7 hard part 6 (i));
      * oracle equality on a 1M-row prefix index holding the same first rows (hard part 6 (iii))."""
    import torch
    from compare import assert_topk_parity
    from oracle import svs_oracle as oracle
    n, d, k = 12_500_000, 1536, 100
    off = 7 * n                                   # global row of local row 0 on rank 7
    qs = _queries(64, d, 31)
    rows_2_31 = (1 << 31) // d                    # first row past element offset 2^31
    rows_2_32 = (1 << 32) // d
    plant_at = [5, rows_2_31 - 1, rows_2_31 + 1, rows_2_32 + 2, 6_250_000, n - 3]
    planted = {r: qs[i].clone() for i, r in enumerate(plant_at)}
    idx = _build_in_blocks(n, d, "f16", 7171, planted, row_offset=off)
    assert idx.hbm_bytes >= n * d * 2 and idx.row_offset == off
    qh = qs.cpu().numpy()
    singles = []
    for qi in range(16):
        one = idx.search(qh[qi], k)
        singles.append(one)
        if qi < len(plant_at):
            assert one[0][1] == off + plant_at[qi] and abs(one[0][0] - 1.0) < 2e-3, (qi, one[0])
    bs, br = idx.search_batch(qh[:16], k)
    for qi in range(16):
        _same_up_to_near_ties(bs[qi], br[qi], np.array([s for s, _ in singles[qi]], dtype=np.float32),
                              np.array([r for _, r in singles[qi]], dtype=np.int64), 4e-6)
    ts, tr = idx.search_batch(qh, k)              # 64 queries: tiled MFMA kernel, fused epilogue
    for qi in (0, 3, 5, 40, 63):
        one = singles[qi] if qi < 16 else idx.search(qh[qi], k)
        _same_up_to_near_ties(ts[qi], tr[qi], np.array([s for s, _ in one], dtype=np.float32),
                              np.array([r for _, r in one], dtype=np.int64), 4e-6)
    assert tr.min() >= off and tr.max() < off + n
    # host recomputation of the returned rows' scores from regenerated rows (query 9: no planted row)
    got = singles[9]
    q16 = qh[9].astype(np.float16).astype(np.float64)
    for s, r in got[:10] + got[-5:]:
        row = _block_rows(n, d, 7171, r - off, r - off + 1)[0].astype(np.float16).astype(np.float64)
        assert abs(float(row @ q16) - s) < 1e-5, (r, s)
    # count-above-threshold check on the WHOLE shard (SURVEY section 7 hard part 6 (ii)): the full score vector of
    # the same kernel (svs_index_scores: 12.5M f32 = 50 MB, read back once) holds exactly k - 1 scores above the
    # returned k-th one and the returned scores are its k largest -- nothing anywhere in the 38 GB was missed
    for qi in (9, 3):
        full = idx.scores(qh[qi])
        assert full.shape == (n,)
        got = singles[qi]
        kth = np.float32(got[-1][0])
        above, at_least = int(np.count_nonzero(full > kth)), int(np.count_nonzero(full >= kth))
        assert above <= k - 1 < at_least, (qi, above, at_least)
        assert above == k - 1 or len({s for s, _ in got}) < k          # exactly k - 1 unless scores tie
        top = np.sort(full[np.argpartition(full, -k)[-k:]])[::-1]
        assert np.array_equal(top, np.array([s for s, _ in got], dtype=np.float32)), f"query {qi}: the k largest scores of the shard"
        assert all(full[r - off] == np.float32(s) for s, r in got[:5] + got[-5:])
        del full
    idx.release()
    torch.cuda.empty_cache()
    # oracle equality on a <= 1M-row prefix index of the same corpus
    pre_n = 1_000_000
    pre = _build_in_blocks(pre_n, d, "f16", 7171, {r: v for r, v in planted.items() if r < pre_n})
    md = pre.stored_rows()
    for qi in (0, 9):
        qd = pre.stored_query(qh[qi])
        got = pre.search(qh[qi], k)
        exp = oracle.cpu_search(md, qd, k)
        assert_topk_parity([s for s, _ in got], [r for _, r in got], [s for s, _ in exp], [r for _, r in exp],
                           oracle.cpu_scores_f64(md, qd), label=f"configs[3] prefix q{qi}")
    pre.release()


def test_config3_shard_row_offset_and_merge(gpu):
    """configs[3]'s exchange on one card: two shards with the row offsets of ranks 6 and 7 of 8
    (global rows beyond 75M) return GLOBAL rows, and their host merge equals one index over both --
    the G-independence argument of SURVEY 8(e) at the f16 dtype."""
    import torch
    from svs_amd import DeviceIndex
    from svs_amd.sharded import merge_topk
    n, d, k = 200_000, 1536, 100
    base = 6 * 12_500_000
    qs = _queries(4, d, 32).cpu().numpy()
    ga, gb = _corpus(n, d, 8181), _corpus(n, d, 8182)
    sa = DeviceIndex.from_device_pointer(ga.data_ptr(), n, d, device=0, row_offset=base, dtype="f16")
    sb = DeviceIndex.from_device_pointer(gb.data_ptr(), n, d, device=0, row_offset=base + n, dtype="f16")
    both = torch.cat([ga, gb])
    whole = DeviceIndex.from_device_pointer(both.data_ptr(), 2 * n, d, device=0, row_offset=base, dtype="f16")
    torch.cuda.synchronize()
    for q in qs:
        la, lb = sa.search(q, k), sb.search(q, k)
        ms, mr = merge_topk(np.array([s for s, _ in la + lb], dtype=np.float32), np.array([r for _, r in la + lb]), k)
        w = whole.search(q, k)
        assert [int(r) for r in mr] == [r for _, r in w] and [float(s) for s in ms] == [s for s, _ in w]
        assert min(r for _, r in w) >= base
    for x in (sa, sb, whole):
        x.release()


def test_config4_fp8_10m_rows_b256(gpu):
    """BASELINE configs[4] at its stated size: 10M x 3072 fp8 (30.7 GB + 40 MB of row scales),
    256 queries per call, v_mfma_f32_16x16x128_f8f6f4 tiles with the fused top-k epilogue.
    Built in device blocks (the 123 GB f32 source never exists).
      * fused == materialised (set_variant(6)), bit for bit, 256 queries x top-100;
      * planted rows (first tile, past byte offset 2^32, last tile) come first;
      * a single-query search (streaming kernel, other summation order) agrees up to near ties;
      * host recomputation of returned scores from regenerated, re-quantised rows."""
    import torch
    n, d, k, nq = 10_000_000, 3072, 100, 256
    qs = _queries(nq, d, 23)
    rows_2_32 = (1 << 32) // d
    plant_at = [3, rows_2_32 + 1, 9_999_998]
    planted = {r: qs[10 + i].clone() for i, r in enumerate(plant_at)}
    idx = _build_in_blocks(n, d, "fp8", 6262, planted)
    assert idx.hbm_bytes == n * d + 4 * n
    qh = qs.cpu().numpy()
    fs, fr = idx.search_batch(qh, k)
    for i, r in enumerate(plant_at):
        assert fr[10 + i, 0] == r and abs(fs[10 + i, 0] - 1.0) < 0.02, (r, fr[10 + i, 0], fs[10 + i, 0])   # e4m3 rounding
    assert np.all(np.diff(fs, axis=1) <= 0) and fr.min() >= 0 and fr.max() < n
    idx.set_variant(6)
    for q0 in range(0, nq, 64):                   # 64 queries x 10M rows x 4 B = 2.56 GB of scores at a time
        ms, mr = idx.search_batch(qh[q0:q0 + 64], k)
        assert np.array_equal(mr, fr[q0:q0 + 64]) and np.array_equal(ms, fs[q0:q0 + 64]), f"queries {q0}.."
    idx.set_variant(0)
    for qi in (0, 100, 255):   # (not the planted queries: a score of 1.0 is 3072 same-sign products, and the two
        one = idx.search(qh[qi], k)   #  f32 summation orders differ by ~1e-5 there; ordinary scores are ~0.09)
        _same_up_to_near_ties(fs[qi], fr[qi], np.array([s for s, _ in one], dtype=np.float32),
                              np.array([r for _, r in one], dtype=np.int64), 4e-6)
    # count-above-threshold on the whole 10M-row corpus (hard part 6 (ii)) through the single-query kernel
    one = idx.search(qh[100], k)
    full = idx.scores(qh[100])
    kth = np.float32(one[-1][0])
    above, at_least = int(np.count_nonzero(full > kth)), int(np.count_nonzero(full >= kth))
    assert above <= k - 1 < at_least, (above, at_least)
    assert np.array_equal(np.sort(full[np.argpartition(full, -k)[-k:]])[::-1], np.array([s for s, _ in one], dtype=np.float32))
    del full
    # host recomputation: the stored row (dequantised by the library) against the library's view of the query
    qd = idx.stored_query(qh[0]).astype(np.float64)
    for j in (0, 1, 50, 99):
        r = int(fr[0, j])
        assert abs(float(idx.stored_rows(r, 1)[0].astype(np.float64) @ qd) - float(fs[0, j])) < 1e-5
    # ... and the stored row itself against an independent quantisation of the regenerated f32 row
    r = int(fr[0, 0])
    raw = _block_rows(n, d, 6262, r, r + 1)[0]
    scale = np.float32(np.abs(raw).max()) / np.float32(448.0)
    ext = torch.from_numpy((raw * (np.float32(1.0) / scale)).astype(np.float32)).to(torch.float8_e4m3fn).to(torch.float32).numpy() * scale
    assert np.mean(ext != idx.stored_rows(r, 1)[0]) < 2e-3
    idx.release()

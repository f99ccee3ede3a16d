"""GPU: every batched score kernel the library ships, each at the shapes that reach it (tests/batch_kernel_table.py),
checked two ways:

  * materialised forms: search_batch(Q, k = n) ranks every row, so the whole (nq, n) score matrix comes back; every
    element is compared with the product of the STORED corpus and the STORED queries in f64;
  * fused forms: a Gaussian corpus with planted rows in every 256-row tile (both sides of every seam, rows 0 and n - 1,
    one varying position inside each tile) -- every planted row must come back, for every query, and each top-k must
    match the oracle's on the stored corpus and, bit for bit, the materialised run of the same kernel (variant 6).

Every case first asserts, through svs_internal_last_launches, that its main pass ran the kernel the table names: a case
that silently reaches another kernel tests nothing it claims to."""
import ctypes

import numpy as np
import pytest

from batch_kernel_table import AB_ONLY, CASES, FUSED, MAT, NF1, NORMS, _ab_shape, case_id
from compare import assert_topk_parity
from oracle import svs_oracle as oracle
from synth import corpus_and_query

pytestmark = pytest.mark.gpu

# |score - f64| on unit-norm rows and queries: the bounds of test_dims_gpu.py -- except for the fp8 MFMA kernels.
# v_mfma_f32_16x16x128_f8f6f4 sums each 128-byte k-group carrying ~13 bits below its LARGEST product,
# so its error scales with the largest component product, not with the score: short rows have large components.  Measured
# on these cases: 9.24e-6 at d = 128 (gemm_tiled_kernel<128, false, 1, 256>, 5,119 rows x 65 queries), 5.84e-6 at d = 256
# (gemm_tiled_kernel<256, false, 1, 256>, 3,000 x 129), at most 5e-6 at d >= 768.  They are held to compare.SCORE_ATOL,
# the bar every fp8 batch top-k test meets; the single-query fp8 kernels (f32 FMAs, the "gemv" rows) to 5e-6.
TOL = {"f32": 2e-6, "f16": 2e-6, "fp8": 1e-5}
TOL_FP8_GEMV = 5e-6
QMAX = 513      # queries drawn per fused corpus (each case takes the first nq)


def _stored_queries(qs, dtype):
    """The queries as the kernels see them: rounded / quantised exactly as rows of an index of that dtype are
    (svs_index_debug_query builds a one-row index for the same reason)."""
    from svs_amd import DeviceIndex
    if dtype == "f32":
        return qs
    qi = DeviceIndex(qs, dtype=dtype)
    out = qi.stored_rows()
    qi.release()
    return out


def _f64_scores(md, qd, block=16384):
    """(n, nq) = md @ qd.T accumulated in f64, computed in row blocks."""
    q64 = qd.astype(np.float64).T
    out = np.empty((md.shape[0], qd.shape[0]))
    for r0 in range(0, md.shape[0], block):
        out[r0:r0 + block] = md[r0:r0 + block].astype(np.float64) @ q64
    return out


def _main_pass(n, nq, kernel, fused):
    """The kernel the last search on this thread ran over all n rows (the fused path's threshold pass covers fewer)."""
    from svs_amd import _native
    launches = _native.last_launches()
    main = [rec for rec in launches if rec[1] == n]
    assert main, f"no launch over all {n} rows: {launches}"
    assert main[0][0] == kernel, f"main pass ran {main[0][0]}, the table says {kernel} (all launches: {launches})"
    assert main[0][2] == nq or kernel.startswith("gemm_q16r_kernel"), launches   # (q16: one launch per 16 queries)
    if fused:
        assert launches[0][1] < n, f"a fused search starts with its threshold pass over a sample: {launches}"
    else:
        assert all(rec[1] == n for rec in launches), f"a materialised search has no threshold pass: {launches}"
    return launches


# ---- materialised forms: the whole score matrix against f64 ---------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c[5] in (MAT, NORMS)], ids=case_id)
def test_materialised_score_matrix_vs_f64(gpu, case):
    from svs_amd import DeviceIndex
    dtype, d, n, nq, k, form, kernel = case
    assert k == n
    m, qs = corpus_and_query("gaussian", 5000 + d + nq + n % 997, n, d, nq)
    if form == NORMS:
        rng = np.random.default_rng(d + nq)
        m *= (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)[:, None]
        qs *= (10.0 ** rng.uniform(-1, 1, nq)).astype(np.float32)[:, None]
    idx = DeviceIndex(m, dtype=dtype)
    s, r = idx.search_batch(qs, k)
    _main_pass(n, nq, kernel, fused=False)
    md = m if dtype == "f32" else idx.stored_rows()
    idx.release()
    assert s.shape == (nq, n) and r.shape == (nq, n)
    # every row list is a permutation of 0..n-1, in (score desc, row desc) order
    assert np.array_equal(np.sort(r, axis=1), np.broadcast_to(np.arange(n), (nq, n))), "row lists are not permutations"
    ds = np.diff(s, axis=1)
    assert np.all(ds <= 0) and np.all(np.diff(r, axis=1)[ds == 0] < 0), "not in (score desc, row desc) order"
    got = np.empty((nq, n))
    np.put_along_axis(got, r, s.astype(np.float64), axis=1)
    qd = _stored_queries(qs, dtype)
    err = np.abs(got - _f64_scores(md, qd).T)
    tol = TOL_FP8_GEMV if dtype == "fp8" and kernel == "gemv" else TOL[dtype]
    if form == NORMS:
        scale = np.linalg.norm(qd.astype(np.float64), axis=1)[:, None] * np.linalg.norm(md.astype(np.float64), axis=1)[None, :]
        rel = err / scale
        q, row = np.unravel_index(np.argmax(rel), rel.shape)
        assert rel[q, row] <= tol, (f"{kernel} {dtype} d={d}: |err| = {err[q, row]:.3g} at query {q}, row {row} "
                                    f"= {rel[q, row]:.3g} x |row| |q| (bound {tol})")
    else:
        q, row = np.unravel_index(np.argmax(err), err.shape)
        assert err[q, row] <= tol, f"{kernel} {dtype} d={d} n={n} nq={nq}: max |score - f64| = {err[q, row]:.3g} at query {q}, row {row}"


# ---- fused forms: planted rows that cover every tile ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fused_corpora():
    """{(d, n): (Gaussian background f32 (n, d), QMAX unit queries)}, built once per module."""
    cache = {}

    def get(d, n):
        if (d, n) not in cache:
            cache[(d, n)] = corpus_and_query("gaussian", 7000 + d + n % 1000, n, d, QMAX)
        return cache[(d, n)]
    return get


def _planted_rows(n):
    """Rows 0 and n - 1, both sides of every 256-row seam, and one position inside every 256-row block that moves from
    block to block; sorted, distinct."""
    pos = {0, n - 1}
    for j in range(256, n, 256):
        pos.update((j - 1, j))
    for b0 in range(0, n, 256):
        pos.add(b0 + (b0 // 256 * 37 + 101) % min(256, n - b0))
    return np.array(sorted(pos), dtype=np.int64)


def _plant(m, qs, k, seed):
    """Overwrites the planted rows of m (in place): row i of query owner[i] is a*q + sqrt(1 - a^2)*v, v a random unit
    vector orthogonal to the query, a distinct per query in [0.5, 0.95].  Rows 0 and n - 1 are the SAME vector, for
    query 0.  Returns {query: planted rows}."""
    n, d = m.shape
    nq = qs.shape[0]
    rows = _planted_rows(n)
    rest = rows[(rows != 0) & (rows != n - 1)]
    owner = np.arange(1, rest.size + 1) % nq          # round-robin; query 0 also owns the pair at 0 and n - 1
    per_q = {q: rest[owner == q].tolist() for q in range(nq)}
    per_q[0] += [0, n - 1]
    assert max(len(v) for v in per_q.values()) <= k // 2, "more planted rows per query than k / 2: raise k"
    rng = np.random.default_rng(seed)
    for q, rs in per_q.items():
        if not rs:
            continue
        qh = qs[q].astype(np.float64)
        qh /= np.linalg.norm(qh)
        a = rng.permutation(np.linspace(0.5, 0.95, len(rs)))
        v = rng.standard_normal((len(rs), d))
        v -= np.outer(v @ qh, qh)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        m[rs] = (a[:, None] * qh[None, :] + np.sqrt(1.0 - a * a)[:, None] * v).astype(np.float32)
    m[n - 1] = m[0]                                    # bit-identical pair: row n - 1 must come first
    return per_q


@pytest.mark.parametrize("case", [c for c in CASES if c[5] == FUSED], ids=case_id)
def test_fused_planted_rows_in_every_tile(gpu, fused_corpora, case):
    from svs_amd import DeviceIndex, _native
    dtype, d, n, nq, k, _, kernel = case
    base, qall = fused_corpora(d, n)
    qs = np.ascontiguousarray(qall[:nq])
    m = base.copy()
    planted = _plant(m, qs, k, seed=nq + d)
    idx = DeviceIndex(m, dtype=dtype)
    del m
    s, r = idx.search_batch(qs, k)
    _main_pass(n, nq, kernel, fused=True)
    phases = (ctypes.c_double * 6)()
    assert _native.load().svs_internal_host_phases(phases, 6) == 0
    assert phases[5] == 0, f"{int(phases[5])} queries were re-run through the materialised path"
    assert s.shape == (nq, k)
    assert r.min() >= 0 and r.max() < n
    srt = np.sort(r, axis=1)
    assert np.all(np.diff(srt, axis=1) > 0), "a row appears twice in one query's top-k"
    for q, rs in planted.items():
        missing = set(rs) - set(r[q].tolist())
        assert not missing, f"query {q}: planted rows {sorted(missing)[:10]} missing"
    # the bit-identical pair (query 0): same score, row n - 1 first
    i0, i1 = int(np.nonzero(r[0] == 0)[0][0]), int(np.nonzero(r[0] == n - 1)[0][0])
    assert s[0, i0] == s[0, i1] and i1 < i0
    # the oracle on the stored corpus, every query
    md = idx.stored_rows()
    qd = _stored_queries(qs, dtype)
    t64 = _f64_scores(md, qd).T.copy()                  # (nq, n)
    s32 = np.dot(md, qd.T).T.copy()                     # np.dot of the reference, f32
    del md
    for q in range(nq):
        exp = oracle.cpu_top_k(s32[q], k)
        assert_topk_parity(s[q], r[q], [x for x, _ in exp], [i for _, i in exp], t64[q],
                           label=f"{kernel} {dtype} d={d} nq={nq} q{q}")
    # the materialised run of the same kernel: bit for bit
    idx.set_variant(6)
    s6, r6 = idx.search_batch(qs, k)
    idx.set_variant(0)
    idx.release()
    assert np.array_equal(r6, r) and np.array_equal(s6, s), "fused != materialised run of the same kernel"


# ---- kernels only an A/B variant reaches: the variant the table names reaches them, and they answer correctly --------
@pytest.mark.parametrize("kernel", sorted(AB_ONLY))
def test_ab_only_kernels_reached_by_their_variant(gpu, fused_corpora, kernel):
    from svs_amd import DeviceIndex
    dtype, d, n, nq = _ab_shape(kernel)
    k = 10
    m, qall = fused_corpora(d, n) if n == NF1 else corpus_and_query("gaussian", 8000 + d, n, d, nq)
    qs = np.ascontiguousarray(qall[:nq])
    idx = DeviceIndex(m, dtype=dtype)
    idx.set_variant(AB_ONLY[kernel])
    s, r = idx.search_batch(qs, k)
    _main_pass(n, nq, kernel, fused=n == NF1)
    md = m if dtype == "f32" else idx.stored_rows()
    idx.release()
    qd = _stored_queries(qs[[0, nq - 1]], dtype)
    for j, q in enumerate((0, nq - 1)):
        exp = oracle.cpu_search(md, qd[j], k)
        assert_topk_parity(s[q], r[q], [x for x, _ in exp], [i for _, i in exp], oracle.cpu_scores_f64(md, qd[j]),
                           label=f"{kernel} (variant {AB_ONLY[kernel]}) q{q}")

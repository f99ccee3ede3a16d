"""GPU: every single-query score kernel the library ships, each at a shape that reaches it
(tests/single_kernel_table.py), through DeviceIndex.scores -- svs_index_scores_n: launch_scores under the index's
variant, no select stage behind it.  Every call first asserts that svs_internal_last_launches reads exactly
[("gemv", n, 1), (kernel, n, 1)]: a case that silently reaches another kernel tests nothing it claims to.

Three properties, for every kernel:
  * f64 closeness: max |score - f64| on what the index really stores, at the bounds of test_dims_gpu.py (unit-norm
    rows; relative to |row| |q| on rows whose norms span 1e-2 .. 1e2), at n = 2 B + G + 1 (several workgroups, full
    groups, a partial last group and wave), n = 1 and n = G - 1 (every clamped lane re-reads row n - 1);
  * exact one-hot products: row i holds one value, at column i mod d; its score is that value times the query's, to the
    bit (f32, f16) -- any chunk read against the wrong query chunk shows, whatever d;
  * position- and variant-independent bits: one row copied n times scores with one bit pattern, and the f32 rows of
    whole wave loads score the same bits under variants 0 .. 5 (gemv_f32.h: "a row's score bits do not depend on which
    of them ran").
Then the loops small n never enters (the persistent kernel's double-buffered loop with both tails, a second trip of the
grid-stride kernels), non-finite values in a row's last chunk, and the query staging of pad_query."""
import zlib

import numpy as np
import pytest

from oracle import svs_oracle as oracle
from single_kernel_table import CASES, LONG_ROWS, LOOP, LOOPS, PER16, case_id, choose_ld, rows_per_block, rows_per_wave

pytestmark = pytest.mark.gpu

# |score - f64| on unit-norm rows and queries: the bounds of test_dims_gpu.py (and, for the single-query fp8 kernels,
# TOL_FP8_GEMV of test_batch_kernels_gpu.py)
TOL = {"f32": 2e-6, "f16": 2e-6, "fp8": 5e-6}
KERNEL = {(dtype, d, variant): kernel for dtype, d, variant, kernel in CASES}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _unit(rng, n, d):
    x = rng.standard_normal((n, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def _open(m, dtype, variant):
    from svs_amd import DeviceIndex
    idx = DeviceIndex(m, dtype=dtype)
    assert idx.ld == choose_ld(m.shape[1], dtype), (dtype, m.shape[1], idx.ld)
    idx.set_variant(variant)
    return idx


def _scores(idx, q, kernel):
    """idx.scores(q), having asserted which kernel computed them."""
    from svs_amd import _native
    got = idx.scores(q)
    launches = _native.last_launches()
    assert launches == [("gemv", idx.n, 1), (kernel, idx.n, 1)], \
        f"{idx.dtype} d={idx.d} ld={idx.ld} n={idx.n}: launched {launches}, the table says {kernel}"
    assert got.shape == (idx.n,)
    return got


def _stored(idx, m, qs):
    """Rows and queries as the kernels see them."""
    if idx.dtype == "f32":
        return m, qs
    return idx.stored_rows(), np.stack([idx.stored_query(q) for q in qs])


def _check_f64(m, qs, dtype, variant, kernel, relative=False):
    idx = _open(m, dtype, variant)
    try:
        md, qd = _stored(idx, m, qs)
        md64 = md.astype(np.float64)
        for j, q in enumerate(qs):
            got = _scores(idx, q, kernel)
            err = np.abs(got.astype(np.float64) - md64 @ qd[j].astype(np.float64))
            if relative:
                err /= np.linalg.norm(md64, axis=1) * np.linalg.norm(qd[j].astype(np.float64))
            row = int(np.argmax(err))
            assert err[row] <= TOL[dtype], (f"{kernel} {dtype} d={idx.d} n={idx.n} query {j}: max |score - f64| "
                                            f"{'/ (|row| |q|) ' if relative else ''}= {err[row]:.3g} at row {row}")
    finally:
        idx.release()


def _edge_sizes(kernel):
    g, b = rows_per_wave(kernel), rows_per_block(kernel)
    return sorted({2 * b + g + 1, 1, max(g - 1, 1)}, reverse=True)


# ---- a. edges: several workgroups and a partial last group; one row; one row short of a wave's group -----------------
@pytest.mark.parametrize("case", CASES + LONG_ROWS, ids=case_id)
def test_edges_vs_f64(gpu, case):
    dtype, d, variant, kernel = case
    rng = np.random.default_rng(_seed("edges", case))
    sizes = _edge_sizes(kernel)
    for n in sizes:
        _check_f64(_unit(rng, n, d), _unit(rng, 2, d), dtype, variant, kernel)
    # row norms 1e-2 .. 1e2, query norms 1e-1 .. 1e1: the same numbers, relative to |row| |q|
    n = sizes[0]
    m, qs = _unit(rng, n, d), _unit(rng, 2, d)
    m *= (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)[:, None]
    qs *= (10.0 ** rng.uniform(-1, 1, 2)).astype(np.float32)[:, None]
    _check_f64(m, qs, dtype, variant, kernel, relative=True)


# ---- b. one non-zero per row ------------------------------------------------------------------------------------------
def _away_from_zero(rng, size):
    """Gaussian values with |x| >= 1/64: every value, its half rounding and every product of two are normal numbers, so
    an exact product says where the kernel read, not how a denormal mode is set."""
    x = rng.standard_normal(size, dtype=np.float32)
    return np.copysign(np.maximum(np.abs(x), np.float32(1 / 64)), x)


BLOCK_ELEMS = 1 << 24      # one-hot corpora are uploaded and read back in blocks of at most 64 MiB


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_one_nonzero_per_row(gpu, case):
    from svs_amd import DeviceIndex
    dtype, d, variant, kernel = case
    rng = np.random.default_rng(_seed("onehot", case))
    n = max(d, 2 * rows_per_block(kernel) + rows_per_wave(kernel) + 1)     # n >= d: every column is some row's
    vals = _away_from_zero(rng, n)
    col = np.arange(n) % d
    q = _unit(rng, 1, d)[0] if dtype == "fp8" else _away_from_zero(rng, d)
    block = max(BLOCK_ELEMS // d, 1)
    idx = DeviceIndex.empty(d, dtype=dtype, reserve=n)
    try:
        for r0 in range(0, n, block):
            nr = min(block, n - r0)
            m = np.zeros((nr, d), dtype=np.float32)
            m[np.arange(nr), col[r0:r0 + nr]] = vals[r0:r0 + nr]
            idx.append(m)
        assert idx.n == n and idx.ld == choose_ld(d, dtype)
        idx.set_variant(variant)
        got = _scores(idx, q, kernel)
        stored = np.empty(n, dtype=np.float32)       # stored[i] = the stored row i at its column
        for r0 in range(0, n, block):
            nr = min(block, n - r0)
            md = vals[r0:r0 + nr, None] if dtype == "f32" else idx.stored_rows(r0, nr)
            if dtype != "f32":
                assert np.count_nonzero(md) == nr, "a stored one-hot row has more than one non-zero"
                md = md[np.arange(nr), col[r0:r0 + nr]]
            stored[r0:r0 + nr] = md.reshape(nr)
        qd = q if dtype == "f32" else idx.stored_query(q)
    finally:
        idx.release()
    want = stored * qd[col]                           # one f32 product per row
    if dtype == "fp8":       # (sum * row scale) * query scale: two more roundings -- the f64 bound, relative to |row| |q|
        err = np.abs(got.astype(np.float64) - stored.astype(np.float64) * qd[col].astype(np.float64))
        err /= np.abs(stored.astype(np.float64)) * np.linalg.norm(qd.astype(np.float64))
        bad = np.flatnonzero(~(err <= TOL["fp8"]))
    else:                    # adding zeros is exact, and so is a product of two halves in f32
        bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{kernel} {dtype} d={d} n={n}: {bad.size} rows wrong, the first row {bad[0]} (column {col[bad[0]]}): "
                           f"score {got[bad[0]]!r}, stored row value x query value = {want[bad[0]]!r}")


# ---- c. the same row everywhere ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + LONG_ROWS, ids=case_id)
def test_identical_rows_score_identical_bits(gpu, case):
    dtype, d, variant, kernel = case
    rng = np.random.default_rng(_seed("same", case))
    row, qs = _unit(rng, 1, d), _unit(rng, 2, d)
    for n in _edge_sizes(kernel):
        idx = _open(np.repeat(row, n, axis=0), dtype, variant)
        try:
            for j, q in enumerate(qs):
                bits = _scores(idx, q, kernel).view(np.uint32)
                odd = np.flatnonzero(bits != bits[0])
                assert odd.size == 0, (f"{kernel} {dtype} d={d} n={n} query {j}: {odd.size} copies of one row score other bits "
                                       f"than row 0 ({bits[0]:#x}), the first row {odd[0]} ({bits[odd[0]]:#x})")
        finally:
            idx.release()


@pytest.mark.parametrize("nstep", range(1, 17))
def test_f32_wave_rows_score_the_same_bits_under_every_variant(gpu, nstep):
    """Variants 0 .. 5 are six launch geometries of two kernels; all sum a row through row_dot_f32."""
    d, n = 256 * nstep, 2 * 64 + 4 + 1
    rng = np.random.default_rng(_seed("variants", nstep))
    m, qs = _unit(rng, n, d), _unit(rng, 2, d)
    m[1::2] = m[1]                                       # and every other row is one row
    idx = _open(m, "f32", 0)
    try:
        ran = set()
        for j, q in enumerate(qs):
            ref = None
            for variant in range(6):
                idx.set_variant(variant)
                kernel = KERNEL.get(("f32", d, variant), KERNEL[("f32", d, 0)])
                bits = _scores(idx, q, kernel).view(np.uint32)
                ran.add(kernel)
                ref = bits if ref is None else ref
                odd = np.flatnonzero(bits != ref)
                assert odd.size == 0, f"{kernel} (variant {variant}) query {j}: row {odd[0]} scores {bits[odd[0]]:#x}, under variant 0 {ref[odd[0]]:#x}"
                assert np.all(bits[1::2] == bits[1]), f"{kernel} (variant {variant}) query {j}: copies of row 1 differ"
        assert len(ran) >= 5, ran
    finally:
        idx.release()


# ---- d. loops that small n never enters -------------------------------------------------------------------------------
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("nstep", [1, 6])
def test_persistent_kernel_steady_state_loop_and_both_tails(gpu, nstep, variant):
    """gemv_f32_rows_kernel: 4 CUs workgroups of 4 waves, wave w takes tiles w, w + W, ...  With 3.5 W tiles half the waves
    take four (the double-buffered loop once, then the two-tile tail) and half take three (the loop once, then the
    one-tile tail)."""
    r, waves = variant, 16 * _cus()
    d, n = 256 * nstep, r * (3 * waves + waves // 2)
    rng = np.random.default_rng(_seed("persistent", nstep, variant))
    _check_f64(_unit(rng, n, d), _unit(rng, 2, d), "f32", variant, KERNEL[("f32", d, variant)])


@pytest.mark.parametrize("t", [1, 8, 64])
@pytest.mark.parametrize("dtype", ["f32", "f16", "fp8"])
def test_loop_kernels_take_a_second_trip(gpu, dtype, t):
    """The grid-stride kernels launch at most 8 CUs workgroups of 4 waves, 64 / T rows per wave: two full trips of the
    grid and a partial third."""
    d = dict(LOOPS)[t] * PER16[dtype] - 1
    n = 2 * (8 * _cus() * 4 * (64 // t)) + 64 // t + 1
    rng = np.random.default_rng(_seed("trips", dtype, t))
    _check_f64(_unit(rng, n, d), _unit(rng, 2, d), dtype, 4, LOOP[dtype].format(t))


# ---- e. non-finite values where the row ends --------------------------------------------------------------------------
NONFINITE_DIMS = [("f32", d) for d in (12, 100, 260, 768, 256, 512)] + [("f16", d) for d in (12, 100, 260, 768, 512)]


@pytest.mark.parametrize("dtype,d", NONFINITE_DIMS)
def test_nonfinite_values_at_the_ends_of_a_row(gpu, dtype, d):
    """One of +inf, -inf, NaN in column 0, a middle column or column d - 1 of single rows.  The lanes of
    gemv_unrolled_kernel / gather_scores_kernel past the end of a row must add exactly nothing, whatever the row's last
    chunk holds: a row's score is np.dot's on the stored values -- +-inf where that is +-inf, NaN only where that is NaN."""
    n, k = 300, 10
    rng = np.random.default_rng(_seed("nonfinite", dtype, d))
    m, qs = _unit(rng, n, d), _unit(rng, 2, d)
    cols = (0, d // 2, d - 1)
    big = {"f32": np.inf, "f16": 1e5}[dtype]             # (f16 ingest turns |x| > 65504 into inf)
    plant = [(row, col, val) for row, (val, col) in zip((0, 7, 64, 65, 130, 200, 255, 256, n - 1),
                                                        [(v, c) for v in (big, -big, np.nan) for c in cols])]
    for row, col, val in plant:
        m[row, col] = val
    qs[0, list(cols)] = (np.abs(qs[0, list(cols)]) + np.float32(1e-3)) * np.array([1, -1, 1], dtype=np.float32)   # non-zero, both signs
    qs[1, d - 1] = 0.0
    idx = _open(m, dtype, 0)
    try:
        md, qd = _stored(idx, m, qs)
        for row, col, val in plant:
            assert (np.isnan(md[row, col]) if np.isnan(val) else md[row, col] == np.sign(val) * np.inf), (row, col, md[row, col])
            assert np.count_nonzero(~np.isfinite(md[row])) == 1
        assert qd[1, d - 1] == 0 and np.all(qd[0, list(cols)] != 0)
        everything = np.arange(n)
        tops = []
        for j, q in enumerate(qs):
            with np.errstate(all="ignore"):
                want = np.dot(md, qd[j])
            got = idx.scores(q)
            label = f"{dtype} d={d} ld={idx.ld} query {j}"
            print(f"{label}: planted rows score {[(r, float(got[r]), float(want[r])) for r, _, _ in plant]} (row, kernel, np.dot)")
            assert np.array_equal(np.isnan(got), np.isnan(want)), \
                f"{label}: NaN at rows {np.flatnonzero(np.isnan(got)).tolist()}, np.dot has it at {np.flatnonzero(np.isnan(want)).tolist()}"
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), \
                f"{label}: infinities {got[np.isinf(got) | inf].tolist()} at rows {np.flatnonzero(np.isinf(got) | inf).tolist()}, np.dot {want[np.isinf(got) | inf].tolist()}"
            fin = np.isfinite(want)
            with np.errstate(all="ignore"):
                t64 = md.astype(np.float64) @ qd[j].astype(np.float64)
            err = np.abs(got[fin].astype(np.float64) - t64[fin])
            assert err.max() <= TOL[dtype], f"{label}: max |score - f64| over the finite rows = {err.max():.3g}"
            top = idx.search(q, k)
            exp = oracle.total_order_top_k(want, k)
            assert [i for _, i in top] == [i for _, i in exp], f"{label}: search returns {top}, the total order on np.dot {exp}"
            assert not top[0][0] == -np.inf
            tops.append([i for _, i in top])
            within = idx.search_within(q, k, everything)
            assert [i for _, i in within] == [i for _, i in top], f"{label}: search_within over every row returns {within}, search {top}"
            # (the gather kernel sums in its own order: the same NaN and infinities, finite scores within the f64 bound)
            ws, wr = np.array([s for s, _ in within]), [i for _, i in within]
            assert np.array_equal(np.isnan(ws), np.isnan(want[wr])) and np.array_equal(ws[np.isinf(ws)], want[wr][np.isinf(want[wr])]), (label, within)
            wfin = np.isfinite(ws)
            assert np.all(np.abs(ws[wfin] - t64[wr][wfin]) <= TOL[dtype]), (label, within)
        # and both queries in one filtered call: the gather kernel's several-queries-per-workgroup form
        _, rb = idx.search_batch_within(qs, k, everything)
        assert rb.tolist() == tops, f"{dtype} d={d}: search_batch_within over every row returns {rb.tolist()}, the single searches {tops}"
    finally:
        idx.release()


# ---- f. query staging -------------------------------------------------------------------------------------------------
def _search_device_all(idx, q_ptr, d):
    """Every score and row of a device-pointer search (k = n), as numpy arrays."""
    import torch
    n = idx.n
    out_s = torch.full((n,), -1.0, device="cuda")
    out_r = torch.full((n,), -1, device="cuda", dtype=torch.int64)
    count = idx.search_device(q_ptr, 1, d, n, out_s.data_ptr(), out_r.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert count == n
    return out_s.cpu().numpy(), out_r.cpu().numpy()


@pytest.mark.parametrize("dtype,d", [("f32", 256), ("f16", 512)])
def test_query_four_bytes_past_a_16_byte_boundary(gpu, dtype, d):
    """The one-shot kernels read the query in 16-byte chunks: pad_query copies one that is not aligned."""
    import torch
    from svs_amd import _native
    n = 300
    rng = np.random.default_rng(_seed("unaligned", dtype, d))
    m, q = _unit(rng, n, d), _unit(rng, 1, d)[0]
    idx = _open(m, dtype, 0)
    try:
        buf = torch.zeros(d + 8, device="cuda")
        aligned, shifted = buf[4:4 + d], buf[1:1 + d]
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        aligned.copy_(torch.from_numpy(q))
        s0, r0 = _search_device_all(idx, aligned.data_ptr(), d)
        assert KERNEL[(dtype, d, 0)] in [rec[0] for rec in _native.last_launches()], _native.last_launches()
        buf.zero_()
        shifted.copy_(torch.from_numpy(q))
        s1, r1 = _search_device_all(idx, shifted.data_ptr(), d)
        assert KERNEL[(dtype, d, 0)] in [rec[0] for rec in _native.last_launches()], _native.last_launches()
        md, qd = _stored(idx, m, q[None, :])
        want = oracle.cpu_scores_f64(md, qd[0])
    finally:
        idx.release()
    assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), "the unaligned query scores differently"
    got = np.empty(n)
    got[r0] = s0
    assert np.max(np.abs(got - want)) <= TOL[dtype]


@pytest.mark.parametrize("dtype,d", [("f32", 250), ("f16", 500)])
def test_kernel_reads_only_the_zero_padded_query_copy(gpu, dtype, d):
    """Rows padded beyond d (250 -> 256 floats, 500 -> 512 halves): the kernel reads ld query floats, which must be the
    padded copy's zeros, never what lies behind the caller's d floats."""
    import torch
    n = 300
    rng = np.random.default_rng(_seed("behind", dtype, d))
    m, q = _unit(rng, n, d), _unit(rng, 1, d)[0]
    idx = _open(m, dtype, 0)
    assert idx.ld > d
    try:
        buf = torch.zeros(idx.ld + 64, device="cuda")
        buf[:d].copy_(torch.from_numpy(q))
        s0, r0 = _search_device_all(idx, buf.data_ptr(), d)
        buf[d:] = float("nan")
        s1, r1 = _search_device_all(idx, buf.data_ptr(), d)
        md, qd = _stored(idx, m, q[None, :])
        want = oracle.cpu_scores_f64(md, qd[0])
    finally:
        idx.release()
    assert not np.isnan(s1).any(), f"{np.isnan(s1).sum()} scores are NaN: the kernel read past the query's {d} floats"
    assert np.array_equal(r0, r1) and np.array_equal(s0.view(np.uint32), s1.view(np.uint32))
    got = np.empty(n)
    got[r0] = s0
    assert np.max(np.abs(got - want)) <= TOL[dtype]

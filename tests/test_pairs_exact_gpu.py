"""GPU: svs_index_top_pairs, both of its paths, against an exact reference, with the kernel each launch reached.

The corpora (tests/pair_cases.py) hold small integers, so every score is exact in every dtype and summation order and
the comparison has no tolerance: the same pairs at the same positions, score bits equal float32(reference), no pair
twice.  Exact duplicates sit on every seam of the pair-mode index arithmetic, and k cuts a tie group, so a wrong tie
order, a pair counted twice and a pair lost at a seam all change the list.  Every dtype is compared with the f64
reference on both paths -- variant 0 materialises n x n scores, variant 1 forces the tiled pair path (svs_amd.hip
top_pairs_tiled) -- not one path with the other.  svs_internal_last_launches names the kernel of every launch."""
import numpy as np
import pytest

import pair_cases as pc

pytestmark = pytest.mark.gpu

MATERIALISED, TILED = 0, 1   # svs_index_set_variant


def _unfused(kernel):
    return kernel.replace("true", "false", 1)


def _expected_launches(kernel, n, P, variant):
    """[(kernel, rows, nq)] of one svs_index_top_pairs call on n > 1024 rows without A/B variants of the kernels."""
    if variant == MATERIALISED:
        return [(_unfused(kernel), n, min(1024, n - q)) for q in range(0, n, 1024)]
    prefix = [(_unfused(kernel), P, min(1024, P - q)) for q in range(0, P, 1024)]          # one launch per prefix chunk
    return prefix + [(kernel, n - rb, 1024) for _, rb, _ in pc.pair_chunks(n)]             # one per query chunk


def _top_pairs(idx, k, variant):
    from svs_amd import _native
    idx.set_variant(variant)
    got = idx.top_pairs(k)
    return got, _native.last_launches()


@pytest.fixture(scope="module", params=pc.CASE_IDS)
def built(request, gpu):
    """(case, index): the corpus is stored once and the reference computed once for both variants."""
    from svs_amd import DeviceIndex
    case = pc.build_case(request.param)
    idx = DeviceIndex(case.rows, dtype=case.dtype)
    pc.check_stored(idx, case.rows)
    case.expected
    yield case, idx
    idx.release()


# ---- a, b: both paths against the reference, and the kernel each launch reached ------------------------------------
@pytest.mark.parametrize("variant", [MATERIALISED, TILED], ids=["materialised", "tiled"])
def test_path_equals_reference(built, variant):
    case, idx = built
    got, launches = _top_pairs(idx, case.k, variant)
    exp = _expected_launches(case.kernel, case.n, case.P, variant)
    assert launches == exp, (launches, exp)
    if variant == MATERIALISED:
        assert all(rows >= case.n for _, rows, _ in launches)
    pc.assert_exact(got, case.expected)


# ---- f: row_offset ---------------------------------------------------------------------------------------------------
def test_row_offset(gpu):
    from svs_amd import DeviceIndex
    case = pc.build_case("f16-d512")
    idx = DeviceIndex(case.rows, dtype=case.dtype, row_offset=1_000_003)
    try:
        for variant in (MATERIALISED, TILED):
            got, launches = _top_pairs(idx, case.k, variant)
            assert launches == _expected_launches(case.kernel, case.n, case.P, variant)
            pc.assert_exact(got, case.expected, row_offset=1_000_003)
    finally:
        idx.release()


# ---- e: tombstones ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tomb_case():
    return pc.build_case("fp8-d128")


def test_tombstoned_winners(gpu, tomb_case):
    """Rows of planted winners are masked: at both ends of the corpus, of a chunk, of the prefix block and in the
    moved-back last chunk.  Both paths must equal the reference over the live rows, in the original row numbers."""
    from svs_amd import DeviceIndex
    case = tomb_case
    qs, q0 = pc.last_chunk(case.n)
    dead = sorted({0, 1023, 2048, 2050, 3074, case.P, case.P - 3, qs, q0 - 1, case.n - 2})
    assert all(any(r in p for p in case.planted) for r in dead)
    ref = pc.reference_on_live(case.rows, dead, case.nominal_k + pc.K_MARGIN)
    k = pc.tie_cut_k(ref, case.nominal_k)
    idx = DeviceIndex(case.rows, dtype=case.dtype)
    try:
        idx.mask_rows(dead)
        for variant in (MATERIALISED, TILED):
            got, launches = _top_pairs(idx, k, variant)
            assert launches == _expected_launches(case.kernel, case.n, case.P, variant)
            assert not any(i in dead or j in dead for _, i, j in got)
            pc.assert_exact(got, ref[:k])
    finally:
        idx.release()


def test_tombstones_double_the_prefix(gpu, tomb_case):
    """All but 24 of the first 16,384 rows are masked: 276 live pairs there, fewer than k = 500, so the prefix block
    must double (to the whole corpus).  The answer is the reference over the live rows."""
    from svs_amd import DeviceIndex
    case = tomb_case
    n, P = case.n, case.P
    assert P == 16384
    keep = {0, 1, 1023, 1024, 2048, 2049, 2050, 2051, P - 3, P - 1}
    for r in np.random.default_rng(3).permutation(P):
        if len(keep) < 24:
            keep.add(int(r))
    assert len(keep) == 24
    dead = [r for r in range(P) if r not in keep]
    n_live = n - len(dead)
    assert 24 * 23 // 2 < case.nominal_k < n_live * (n_live - 1) // 2
    ref = pc.reference_on_live(case.rows, dead, case.nominal_k + pc.K_MARGIN)
    k = pc.tie_cut_k(ref, case.nominal_k)
    idx = DeviceIndex(case.rows, dtype=case.dtype)
    try:
        idx.mask_rows(dead)
        got, launches = _top_pairs(idx, k, TILED)
        assert launches == _expected_launches(case.kernel, n, n, TILED), launches       # P doubled: min(n, 32768) = n
        pc.assert_exact(got, ref[:k])
    finally:
        idx.release()


# ---- c: a tile full of survivors -------------------------------------------------------------------------------------
FULL = [("f16", 512, "gemm_phased_kernel<true, 2, 0, 256>"), ("fp8", 768, "gemm_phased_kernel<true, 1, 0, 256>")]


@pytest.mark.parametrize("dtype,d,kernel", FULL, ids=[f"{t}-d{d}" for t, d, _ in FULL])
def test_every_pair_ties(gpu, dtype, d, kernel):
    """3,000 identical rows: all 4.5 M pairs tie at the bound (inside the 8 Mi pair list and one row's candidate list),
    so every tile of the phased kernel is full of survivors and its waves' parking eighths overflow into the
    direct-to-list branch.  The answer is the closed form (2998, 2999), (2997, 2999), (2997, 2998), ..."""
    from svs_amd import DeviceIndex
    n, k = 3000, 1000
    rows, score = pc.identical_rows(n, d, dtype)
    idx = DeviceIndex(rows, dtype=dtype)
    try:
        pc.check_stored(idx, rows)
        got, launches = _top_pairs(idx, k, TILED)
        assert launches == _expected_launches(kernel, n, n, TILED), launches
        pc.assert_exact(got, pc.all_tied_expected(n, k, score))
    finally:
        idx.release()


# ---- d: the refusals ---------------------------------------------------------------------------------------------------
FUSED_ROWS = 131_072 + 29    # plan_search fuses 16 queries from 8 x 16,384 rows on


def _assert_refuses(idx, k, words):
    idx.set_variant(TILED)
    with pytest.raises(NotImplementedError) as e:
        idx.top_pairs(k)
    assert words in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype,d,kernel", FULL, ids=[f"{t}-d{d}" for t, d, _ in FULL])
def test_refuses_more_pairs_than_the_list_holds(gpu, dtype, d, kernel):
    """4,200 identical rows hold 8.8 M pairs at the bound, more than the 8 Mi pair list: NotImplementedError, and the
    handle is as good as new after it -- the materialised path answers, and (after a second refusal and an append up
    to a fusable size) a 16-query fused batch search returns, bit for bit, what a fresh index returns."""
    from svs_amd import DeviceIndex, _native
    n, k = 4200, 1000
    rows, score = pc.identical_rows(n, d, dtype)
    full = np.concatenate([rows, pc.integer_rows(9, FUSED_ROWS - n, d, dtype)])
    queries = pc.integer_rows(10, 16, d, dtype)
    idx = DeviceIndex(rows, dtype=dtype)
    fresh = None
    try:
        _assert_refuses(idx, k, "near-duplicate documents en masse")
        assert [r for r in _native.last_launches() if "true" in r[0]] == \
            [(kernel, n - rb, 1024) for _, rb, _ in pc.pair_chunks(n)]
        got, _ = _top_pairs(idx, k, MATERIALISED)
        pc.assert_exact(got, pc.all_tied_expected(n, k, score))
        _assert_refuses(idx, k, "near-duplicate documents en masse")
        idx.set_variant(0)
        idx.append(full[n:])
        gs, gr = idx.search_batch(queries, 10)
        main = [r for r in _native.last_launches() if r[1] == FUSED_ROWS]
        assert main and all("true" in r[0] for r in main), _native.last_launches()     # the fused epilogue ran
        fresh = DeviceIndex(full, dtype=dtype)
        fs, fr = fresh.search_batch(queries, 10)
        assert np.array_equal(gr, fr) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
        exact = pc.exact_scores(queries, full)
        for q in range(16):
            order = np.lexsort((-np.arange(FUSED_ROWS), -exact[q]))[:10]
            assert list(gr[q]) == list(order) and np.array_equal(gs[q], exact[q][order].astype(np.float32))
    finally:
        idx.release()
        if fresh is not None:
            fresh.release()


@pytest.mark.parametrize("dtype,d", [("f16", 100), ("f32", 100), ("fp8", 100)])
def test_refuses_rows_that_are_not_whole_lines(gpu, dtype, d):
    """d = 100 is stored with rows that are no multiple of 128 bytes (batch_route: no tiled family): the tiled path refuses before
    it launches anything, and the handle then answers a batch search like a fresh index and the materialised path
    exactly.  (No fused search exists for such rows: plan_search fuses only what the batched kernels take.)"""
    from svs_amd import DeviceIndex, _native
    n = 1500
    rows = pc.plant(pc.integer_rows(11, n, d, dtype), [(0, 1), (0, n - 1), (1023, 1024), (255, 512)])
    queries = pc.integer_rows(12, 16, d, dtype)
    ref = pc.reference_top_pairs(rows, 600)
    k = pc.tie_cut_k(ref, 200)
    exp = ref[:k]
    idx = DeviceIndex(rows, dtype=dtype)
    fresh = DeviceIndex(rows, dtype=dtype)
    try:
        pc.check_stored(idx, rows)
        _assert_refuses(idx, k, "whole 128-byte lines")
        assert _native.last_launches() == []
        idx.set_variant(0)
        gs, gr = idx.search_batch(queries, 50)
        fs, fr = fresh.search_batch(queries, 50)
        assert np.array_equal(gr, fr) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
        _assert_refuses(idx, k, "whole 128-byte lines")
        got, _ = _top_pairs(idx, k, MATERIALISED)
        pc.assert_exact(got, exp)
    finally:
        idx.release()
        fresh.release()


# ---- g: tiny corpora under variant 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 16, 17, 33])
@pytest.mark.parametrize("dtype,d", [("f32", 128), ("f16", 128), ("f16", 256)])
def test_tiny_corpora_tiled(gpu, dtype, d, n):
    """Up to 16 rows the one query chunk would take the 16-query kernels (f32 d = 128, f16 d = 256: batch_route),
    which have no pair mode -- they returned (i, i) and both (i, j) and (j, i) -- so svs_index_top_pairs keeps such
    corpora on the materialised path; from 17 rows on the tiled kernels run in pair mode."""
    from svs_amd import DeviceIndex
    rows = pc.integer_rows(20 + n, n, d, dtype)
    if n > 2:
        rows[n - 1] = rows[0]
    k = n * (n - 1) // 2
    exp = pc.reference_top_pairs(rows, k)
    idx = DeviceIndex(rows, dtype=dtype)
    try:
        pc.check_stored(idx, rows)
        got, launches = _top_pairs(idx, k + 5, TILED)
        assert all(i < j for _, i, j in got) and len({(i, j) for _, i, j in got}) == len(got) == k
        pc.assert_exact(got, exp)
        fused = [r for r in launches if "true" in r[0]]
        assert not any(r[0].startswith("gemm_q16") for r in fused), launches
        if n > 16:
            eb = 4 if dtype == "f32" else 2
            assert fused == [(f"gemm_tiled_kernel<{32 if n <= 32 else 64}, true, {eb}, 128>", n, n)], launches
        else:
            assert fused == [], launches
    finally:
        idx.release()

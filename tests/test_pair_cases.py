"""CPU: the exact pair corpora (tests/pair_cases.py) meet the conditions tests/test_pairs_exact_gpu.py relies on."""
import numpy as np
import pytest

import pair_cases as pc


@pytest.fixture(scope="module", params=pc.CASE_IDS)
def case(request):
    return pc.build_case(request.param)


def _brute(rows, k):
    """Every pair of a small corpus, ordered (score desc, i desc, j desc)."""
    m = rows.astype(np.float64)
    s = m @ m.T
    n = len(m)
    allp = [(float(s[i, j]), i, j) for i in range(n) for j in range(i + 1, n)]
    return sorted(allp, key=lambda t: (-t[0], -t[1], -t[2]))[:k]


def test_case_table():
    names = [c[0] for c in pc.CASES]
    assert len(set(names)) == len(names)
    for name, dtype, d, n, k, kernel in pc.CASES:
        assert n % 4 and n % 256 and n % 1024                       # no multiple of the scale vector, a tile or a chunk
        pc.check_exactness_bounds(dtype, d, pc.value_limit(dtype))
        assert pc.prefix_rows(n, k) < n                             # a prefix block shorter than the corpus
        assert (d > 256) == (n < 10000)                             # the larger d only with the smaller n
    pc.check_e4m3_values()
    assert {n % 4 for _, _, _, n, _, _ in pc.CASES} == {1, 2, 3}
    assert {c[4] for c in pc.CASES} == {500, pc.SEL_KMAX + 1}


def test_corpus_is_exact_integers(case):
    m, lim = case.rows, pc.value_limit(case.dtype)
    assert m.dtype == np.float32 and m.shape == (case.n, case.d)
    assert np.array_equal(m, np.rint(m)) and np.abs(m).max() <= lim
    assert 49 * case.d < 2 ** 24
    if case.dtype == "fp8":
        assert (np.abs(m).max(axis=1) == 7).all()                   # every row's scale is 7 / 448 = 2^-6
        scale = np.abs(m).max(axis=1).astype(np.float32) / np.float32(448.0)
        assert (scale == np.float32(2.0 ** -6)).all()
        assert case.d <= 1024
    for i, j in case.planted:
        assert np.array_equal(m[i], m[j])


def test_planted_positions(case):
    n, P, pl = case.n, case.P, set(case.planted)
    qs, q0 = pc.last_chunk(n)
    assert qs == n - 1024 and q0 % 1024 == 0 and q0 < n - 1 <= q0 + 1024 and qs < q0
    assert {(0, 1), (0, n - 1), (n - 2, n - 1)} <= pl
    for r in (0, 255):
        for delta in (1, 255, 256, 257):
            assert any(i % 256 == r and j - i == delta for i, j in pl), (r, delta)
    for c in range(1024, n, 1024):
        assert (c - 1, c) in pl
    for r in range(4):
        for delta in (1, 2, 3):
            assert any(i % 4 == r and j - i == delta and 0 <= i % 1024 < 4 for i, j in pl), (r, delta)
    assert any(j == qs for _, j in pl) and any(i == qs for i, _ in pl)
    assert any(i == q0 - 1 for i, _ in pl) and any(i == q0 for i, _ in pl)
    assert (P - 1, P) in pl and any(i < P - 1 and j > P for i, j in pl)
    assert P in (8192, 16384) and P == pc.prefix_rows(n, case.k)
    # the chunks the library forms: one per 1024 queries, the last moved back, 4-aligned row bases at or below the chunk
    ch = pc.pair_chunks(n)
    assert len(ch) == (n - 2) // 1024 + 1 and ch[-1] == (qs, (qs + 1) & ~3, q0)
    assert all(rb % 4 == 0 and rb <= s + 1 and s <= f for s, rb, f in ch)


def test_expected_list(case):
    exp, ref, k = case.expected, case.reference, case.k
    assert case.nominal_k <= k < len(ref) and len(exp) == k
    assert exp[-1][0] == ref[k][0]                                   # the tie at k is cut
    pairs = [(i, j) for _, i, j in exp]
    assert len(set(pairs)) == k and all(0 <= i < j < case.n for i, j in pairs)
    assert set(case.planted) <= set(pairs)                           # every planted pair is among the winners
    keys = [(-s, -i, -j) for s, i, j in exp]
    assert keys == sorted(keys)
    rows = case.rows.astype(np.float64)
    for s, i, j in exp[:50] + exp[-50:]:
        assert s == float(rows[i] @ rows[j]) and np.float32(s) == s
    tied = sum(1 for s, _, _ in ref if s == exp[-1][0])
    print(f"{case.name}: k = {k}, {tied} entries tied at the k-th score, {len({s for s, _, _ in exp})} distinct scores")
    assert tied >= 2


def test_reference_equals_brute_force():
    """The chunked reference against every pair of a corpus small enough to enumerate, across chunk seams."""
    m = pc.integer_rows(5, 301, 32, "f32")
    pc.plant(m, [(0, 300), (63, 64), (64, 200), (127, 128), (299, 300)])
    for k in (1, 7, 500, 301 * 300 // 2):
        assert pc.reference_top_pairs(m, k, chunk=64) == _brute(m, k)
    live_ref = pc.reference_on_live(m, {0, 64}, 40)
    keep = [r for r in range(301) if r not in (0, 64)]
    assert live_ref == [(s, keep[i], keep[j]) for s, i, j in _brute(m[keep], 40)]


def test_closed_form_of_identical_rows():
    rows, score = pc.identical_rows(9, 64, "fp8")
    assert pc.all_tied_expected(9, 5, score) == [(score, 7, 8), (score, 6, 8), (score, 6, 7), (score, 5, 8), (score, 5, 7)]
    assert pc.all_tied_expected(9, 36, score) == pc.reference_top_pairs(rows, 36)
    # the sizes tests/test_pairs_exact_gpu.py uses: inside the 8 Mi pair list and one row's candidate list, and past it
    assert 3000 * 2999 // 2 < 8 << 20 < 4200 * 4199 // 2 and 4199 < 32768


def test_tiny_corpora():
    for n in (2, 3, 5, 16, 17, 33):
        m = pc.integer_rows(n, n, 128, "f32")
        assert pc.reference_top_pairs(m, n * (n - 1) // 2) == _brute(m, n * (n - 1) // 2)

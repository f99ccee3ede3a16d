"""Every route of the top-k stage (svs_amd/csrc/select.h; run_select / enqueue_prefix / enqueue_select_half), run ALONE
on chosen data through the svs_internal_select_* hooks and compared BIT-EXACT with the exact order: rows equal, score
bits equal, NaN positions equal; no tolerance anywhere.  select_model.py says which route a case takes (held to the case
table on the CPU by test_select_model.py); here the model's verdict is asserted next to the comparison, so a passing case
pins the route it names.  Every case also asserts that the per-query scratch is all zero behind the selection: a stale
word would corrupt the NEXT search on that context, not this one.

References: oracle.total_order_top_k for score vectors (select_model.expected_scores), a sort of the live keys for
candidate lists, the k-th largest key for the k-th-value kernel.
"""
import re

import numpy as np
import pytest

import select_cases as sc
import select_model as sm

pytestmark = pytest.mark.gpu

NEG_INF_BITS = int(np.float32(-np.inf).view(np.uint32))


@pytest.fixture(scope="module")
def index(gpu):
    """The hooks take the device, a search context and the tombstone bitmap from an index; its rows are not read."""
    from svs_amd import DeviceIndex
    idx = DeviceIndex(np.zeros((sc.CAND_INDEX_ROWS, 1), dtype=np.float32))
    idx.mask_rows(np.arange(sc.DEAD_LO, sc.DEAD_HI))
    yield idx
    idx.release()


_vectors = {}


def _vector(table, name):
    """a case's input, generated once and shared (read-only)"""
    if (id(table), name) not in _vectors:
        v = next(c for c in table if c.name == name).gen()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _vectors[(id(table), name)] = v
    return _vectors[(id(table), name)]


def _groups(table):
    """The table's cases by the first word of their names (the sizes n4097 .. n8193 together): one test per group keeps the
    file to a few dozen tests; every case of a group runs, and the failures are reported together by case name."""
    out = {}
    for c in table:
        word = c.name.split("-")[0]
        out.setdefault("sizes" if re.fullmatch(r"n\d+", word) else word, []).append(c)
    return [pytest.param(cases, id=g) for g, cases in out.items()]


def _each(cases, run):
    failures = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            failures.append(f"{c.name} ({c.why}): {str(e)[:400]}")
    assert not failures, "\n".join(failures)


def _assert_exact(got_s, got_r, want_bits, want_rows, label):
    bad = np.flatnonzero(got_r != want_rows)
    assert bad.size == 0, f"{label}: rows differ at {bad[:5].tolist()}: got {got_r[bad[:5]].tolist()}, want {want_rows[bad[:5]].tolist()}"
    got_bits = got_s.view(np.uint32)
    bad = np.flatnonzero(got_bits != want_bits)
    assert bad.size == 0, f"{label}: score bits differ at {bad[:5].tolist()}: got {got_bits[bad[:5]].tolist()}, want {want_bits[bad[:5]].tolist()}"


def _run_scores(index, vs, k, row_offset=0):
    s, r, count, dirty = index.select_scores(np.stack(vs), k, row_offset)
    assert count == min(k, vs[0].size)
    assert dirty == 0, f"{dirty} scratch words left non-zero"
    return s, r


# ---- run_select over score vectors: paths A, B, D -------------------------------------------------------------
@pytest.mark.parametrize("cases", _groups(sc.SCORE_CASES))
def test_scores_route(index, cases):
    def run(case):
        v = _vector(sc.SCORE_CASES, case.name)
        route = sm.route_scores(v, case.k)
        assert route.name == case.route and (case.emit is None or route.emit == case.emit)
        for k in ((case.k,) if case.route != sm.D else (1, v.size, v.size + 3)):
            s, r = _run_scores(index, [v], k)
            _assert_exact(s[0], r[0], *sm.expected_scores(v, k), label=f"k={k}")
    _each(cases, run)


def test_scores_row_offset(index):
    """row_offset = 10^12 is added in 64 bits, on every emit form and on the padding (-1 stays -1)"""
    for name in ("gauss-k100", "gauss-k257", "B-n4097-k4100", "D-n257"):
        case = next(c for c in sc.SCORE_CASES if c.name == name)
        v = _vector(sc.SCORE_CASES, name)
        k = case.k + 3 if case.route == sm.D else case.k
        s, r = _run_scores(index, [v], k, row_offset=10 ** 12)
        _assert_exact(s[0], r[0], *sm.expected_scores(v, k, row_offset=10 ** 12), label=name)


@pytest.mark.parametrize("mix", sorted(sc.SCORE_MIXES), ids=str)
def test_scores_mixed_queries(index, mix):
    """Queries of different routes in ONE call: each against its own reference and against the same vector run alone."""
    names = sc.SCORE_MIXES[mix]
    k = next(c for c in sc.SCORE_CASES if c.name == names[0]).k
    vs = [_vector(sc.SCORE_CASES, nm) for nm in names]
    s, r = _run_scores(index, vs, k)
    for q, (nm, v) in enumerate(zip(names, vs)):
        _assert_exact(s[q], r[q], *sm.expected_scores(v, k), label=f"{mix}[{q}] {nm}")
        s1, r1 = _run_scores(index, [v], k)
        assert r1[0].tolist() == r[q].tolist() and s1[0].view(np.uint32).tolist() == s[q].view(np.uint32).tolist(), nm


def test_scores_path_d_mixed_queries(index):
    vs = [sc.d_vector(257, seed) for seed in (70, 71, 72)]
    vs[1] = -np.abs(vs[1])
    for k in (1, 257, 260):
        s, r = _run_scores(index, vs, k)
        for q, v in enumerate(vs):
            _assert_exact(s[q], r[q], *sm.expected_scores(v, k), label=f"D nq=3 [{q}] k={k}")


def test_scores_routes_back_to_back_on_one_context(index):
    """The scratch invariant across searches: a route that left a word behind would break the NEXT call.  The raw fallback,
    the candidate radix select and the overflow run first, the cheap route last, twice over, all on one context."""
    order = ["negative-k100", "gauss-k100", "ties12000-k100", "gauss-k100", "equal40000-k5", "big-gauss-k100",
             "ties6000-k41", "onebin-k100", "onebin-k257", "gauss-k100"]
    for _ in range(2):
        for name in order:
            case = next(c for c in sc.SCORE_CASES if c.name == name)
            v = _vector(sc.SCORE_CASES, name)
            s, r = _run_scores(index, [v], case.k)
            _assert_exact(s[0], r[0], *sm.expected_scores(v, case.k), label=name)


# ---- select_final_kernel mode 3 over candidate lists -----------------------------------------------------------------
def _run_candidates(index, cases, k_extra=0):
    count, dead = cases[0].count, cases[0].dead
    lists, claims = zip(*[_vector(sc.CAND_CASES, c.name) for c in cases])
    k = count + k_extra
    s, r, dirty = index.select_candidates(list(lists), list(claims), k, count, use_dead=dead)
    assert dirty == 0, f"{dirty} scratch words left non-zero (a marked query's header included)"
    mask = sc.dead_mask() if dead else None
    for q, c in enumerate(cases):
        route = sm.route_candidates(lists[q], claims[q], count, mask)
        assert route.name == c.route
        want_bits, want_rows = sm.expected_candidates(lists[q], claims[q], count, k, mask)
        if route.name == sm.MARKED:
            assert (want_rows == -2).all() and (want_bits == NEG_INF_BITS).all()
        _assert_exact(s[q], r[q], want_bits, want_rows, label=c.name)
    return s, r


@pytest.mark.parametrize("cases", _groups(sc.CAND_CASES))
def test_candidates_route(index, cases):
    _each(cases, lambda case: _run_candidates(index, [case], k_extra=0 if case.count == 256 else 3))


@pytest.mark.parametrize("mix", sorted(sc.CAND_MIXES), ids=str)
def test_candidates_mixed_queries(index, mix):
    cases = [next(c for c in sc.CAND_CASES if c.name == nm) for nm in sc.CAND_MIXES[mix]]
    s, r = _run_candidates(index, cases)
    for q, c in enumerate(cases):
        s1, r1 = _run_candidates(index, [c])
        assert r1[0].tolist() == r[q].tolist() and s1[0].view(np.uint32).tolist() == s[q].view(np.uint32).tolist(), c.name


# ---- prefix_kth_kernel --------------------------------------------------------------------------------------------------
def _run_kth(index, vs, k, misaligned):
    thr, dirty = index.kth_value(np.stack(vs), k, misalign=misaligned)
    assert dirty == 0
    return thr.view(np.uint32).tolist()


@pytest.mark.parametrize("cases", _groups(sc.KTH_CASES))
def test_kth_route(index, cases):
    def run(case):
        v = _vector(sc.KTH_CASES, case.name)
        assert sm.route_kth(v, case.k, case.misaligned).name == case.route
        assert _run_kth(index, [v], case.k, case.misaligned) == [sm.expected_kth_bits(v, case.k)]
    _each(cases, run)


@pytest.mark.parametrize("mix", sorted(sc.KTH_MIXES), ids=str)
def test_kth_mixed_queries(index, mix):
    names, misaligned = sc.KTH_MIXES[mix]
    k = next(c for c in sc.KTH_CASES if c.name == names[0]).k
    vs = [_vector(sc.KTH_CASES, nm) for nm in names]
    assert _run_kth(index, vs, k, misaligned) == [sm.expected_kth_bits(v, k) for v in vs]


def test_hooks_refuse_what_the_kernels_cannot_take(index):
    """The hooks check what would send a kernel out of bounds (they are test code, but a typo must not fault the device)."""
    one = np.zeros((1, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        index.kth_value(one, 9)
    with pytest.raises(ValueError):
        index.select_scores(one, 0)
    keys = sm.make_keys(np.ones(4, dtype=np.float32), np.arange(4))
    with pytest.raises(ValueError):
        index.select_candidates([keys], [5], 4, 4)                    # fewer keys than the claim
    with pytest.raises(ValueError):
        index.select_candidates([keys], [4], 300, 300)                # count past the fused path's 256
    far = sm.make_keys(np.ones(1, dtype=np.float32), [sc.CAND_INDEX_ROWS])
    with pytest.raises(ValueError):
        index.select_candidates([far], [1], 1, 1, use_dead=True)      # a row outside the bitmap

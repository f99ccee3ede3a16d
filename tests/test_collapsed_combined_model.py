"""CPU: the numpy model of the group-combined search (collapsed_combined_model.py) against a brute-force loop over the
definition, the three identities the header states against collapse_model and combine_model, and the case the entry
exists for: a parent whose two chunks cover one facet each."""
import numpy as np
import pytest

import collapse_model
import combine_model
import select_model
from collapsed_combined_model import brute_force, collapsed_combined

F = np.float32


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def _canon(x):
    """Scores as every search returns them: -0.0 as +0.0, any NaN as 0x7fc00000."""
    return select_model.key_score(select_model.score_key(np.asarray(x, dtype=np.float32))).astype(np.float32)


def _same(a, b):
    assert _bits(a[0]) == _bits(b[0])
    assert a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist() and a[3] == b[3]


def _case(seed, n, m):
    """m score vectors with ties, -0.0, +0.0, NaN and infinities sprinkled in; values in runs; some rows dead."""
    rng = np.random.default_rng(seed)
    s = [np.round(rng.standard_normal(n), 1).astype(F) for _ in range(m)]    # rounded: many score ties
    for j in range(m):
        for special in (F(-0.0), F(0.0), F(np.nan), F(np.inf), F(-np.inf)):
            s[j][rng.integers(0, n, 2)] = special
    values = np.repeat(rng.integers(0, 6, n), rng.integers(1, 4, n))[:n].astype(np.uint32)
    dead = rng.random(n) < 0.2
    return s, values, dead


@pytest.mark.parametrize("op", combine_model.OPS)
@pytest.mark.parametrize("m", [1, 2, 3, 8])
def test_model_equals_the_brute_force_loop(op, m):
    for seed in range(4):
        n = 40 + 7 * seed
        s, values, dead = _case(seed * 10 + m, n, m)
        w = None if seed == 0 else np.random.default_rng(seed).choice([-1.5, -1.0, 0.0, 0.5, 1.0, 2.0], m).astype(F)
        for zero_single in (False, True):
            for k in (0, 1, 5, n + 3):
                args = (s, w, op, values, dead, zero_single, k)
                _same(collapsed_combined(*args), brute_force(*args))
    # no column, nothing dead, and everything dead
    s, values, dead = _case(99, 30, m)
    _same(collapsed_combined(s, None, op, None, None, True, 7), brute_force(s, None, op, None, None, True, 7))
    _same(collapsed_combined(s, None, op, None, None, False, 7), brute_force(s, None, op, None, None, False, 7))
    got = collapsed_combined(s, None, op, values, np.ones(30, dtype=bool), True, 7)
    assert got[3] == 0 and len(got[0]) == len(got[1]) == len(got[2]) == 0


def test_identity_one_vector_max_is_the_collapsed_search():
    for seed in range(5):
        s, values, dead = _case(seed, 60, 1)
        for zero_single in (False, True):
            for k in (0, 3, 100):
                got = collapsed_combined(s, None, "max", values, dead, zero_single, k)
                want = collapse_model.collapsed(s[0], values, dead, zero_single, k)
                _same(got, (_canon(want[0]), want[1], want[2], want[3]))


@pytest.mark.parametrize("op", combine_model.OPS)
def test_identity_single_row_groups_are_the_combined_search(op):
    for seed in range(5):
        m = (2, 3, 8, 1, 4)[seed]
        s, _, dead = _case(seed + 20, 50, m)
        for j in range(m):
            s[j][np.isinf(s[j])] = F(1.5)      # (a LIVE row at -inf ties with the masked rows in the row-level search: the header's caveat)
        w = None if seed % 2 else np.random.default_rng(seed).choice([-2.0, -1.0, 0.0, 0.25, 1.0, 3.0], m).astype(F)
        live = int((~dead).sum())
        for k in (0, 4, 50):
            got = collapsed_combined(s, w, op, None, dead, True, k)              # a column never set + "single"
            bits, rows, count = combine_model.top_k(s, w, op, k, np.nonzero(dead)[0])
            assert got[3] == live and len(got[0]) == count == min(k, live)
            assert got[1].tolist() == rows[:count].tolist() and not got[2].any()
            assert _bits(got[0]) == _bits(_canon(bits[:count].view(np.float32)))


def test_identity_max_with_non_negative_weights_commutes_with_collapsing():
    for seed in range(6):
        m = (2, 3, 8)[seed % 3]
        s, values, dead = _case(seed + 40, 70, m)
        for j in range(m):
            s[j][np.isnan(s[j])] = F(0.5)      # (w * NaN is NaN for every w: kept out so that w = 0 stays monotone)
            s[j][np.isinf(s[j])] = F(-3.0)     # (0 * inf is NaN)
        w = None if seed < 2 else np.random.default_rng(seed).choice([0.0, 0.5, 1.0, 2.0], m).astype(F)
        c_row = combine_model.combine(s, w, "max")
        for zero_single in (False, True):
            got = collapsed_combined(s, w, "max", values, dead, zero_single, 70)
            want = collapse_model.collapsed(c_row, values, dead, zero_single, 70)
            _same(got, (_canon(want[0]), want[1], want[2], want[3]))


def test_a_parent_whose_chunks_cover_one_facet_each_wins_under_min():
    # parent 1: chunk 0 answers facet A (0.9 / 0.1), chunk 1 facet B (0.1 / 0.9); parent 2: one lukewarm chunk (0.5 / 0.5)
    s = [np.array([0.9, 0.1, 0.5], dtype=F), np.array([0.1, 0.9, 0.5], dtype=F)]
    values = np.array([1, 1, 2], dtype=np.uint32)
    sc, rows, vals, groups = collapsed_combined(s, None, "min", values, None, True, 2)
    assert groups == 2 and vals.tolist() == [1, 2] and _bits(sc) == _bits([F(0.9), F(0.5)])
    assert rows.tolist() == [1, 2]             # parent 1's rows tie at min = 0.1: the larger row represents it
    # the row-level search ranks them the other way: no single chunk of parent 1 covers both facets
    _, r, _ = combine_model.top_k(s, None, "min", 3)
    assert r.tolist() == [2, 1, 0]
    # "any" (max) and "sum" agree with the chunk level on who is first, but score the parent by both chunks
    assert _bits(collapsed_combined(s, None, "sum", values, None, True, 1)[0]) == _bits([F(0.9) + F(0.9)])

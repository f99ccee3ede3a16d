"""CPU: the numpy model of the threshold search (above_model.py) against brute force -- Python's own ``sorted`` over
(float(score), row) tuples, the order the top-k searches are defined by -- on small vectors with planted ties, signed
zeros, infinities and NaN scores."""
import math

import numpy as np
import pytest

import above_model


def _brute(scores, dead, cut, limit):
    """Plain Python.  NaN scores: they qualify for every cut-off and come first (row descending among themselves), which is
    what the key order says; the rest is ``sorted(reverse=True)`` on (float(score), row) -- float(-0.0) == float(0.0), so
    the tie falls through to the row, as in the key."""
    cut = float(cut)
    live = [r for r in range(len(scores)) if not (dead is not None and dead[r])]
    nans = sorted((r for r in live if math.isnan(float(scores[r]))), reverse=True)
    rest = sorted(((float(scores[r]), r) for r in live if not math.isnan(float(scores[r])) and float(scores[r]) >= cut), reverse=True)
    rows = nans + [r for _, r in rest]
    return rows[:min(max(limit, 0), len(rows))], len(rows)


def _vector(rng, n):
    s = rng.standard_normal(n).astype(np.float32)
    s[rng.choice(n, n // 8, replace=False)] = np.float32(0.25)       # planted ties
    s[rng.choice(n, 4, replace=False)] = [0.0, -0.0, 0.0, -0.0]
    s[rng.choice(n, 4, replace=False)] = [np.inf, -np.inf, np.inf, -np.inf]
    s[rng.choice(n, 2, replace=False)] = np.nan
    return s


def test_score_key_matches_the_header():
    k = above_model.score_key
    assert k(0.0)[0] == k(-0.0)[0] == 0x80000000
    assert k(np.nan)[0] == 0xFFFFFFFF and k(np.float32(np.nan) * -1)[0] == 0xFFFFFFFF
    assert k(-np.inf)[0] == 0x007FFFFF and k(np.inf)[0] == 0xFF800000
    v = np.array([-np.inf, -3.5, -1e-40, 0.0, 1e-40, 0.25, 7.0, np.inf], dtype=np.float32)
    assert (np.diff(k(v).astype(np.int64)) > 0).all()


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = 97 + 13 * seed
    s = _vector(rng, n)
    dead = rng.random(n) < 0.15 if seed % 2 else None
    finite = s[np.isfinite(s)]
    cuts = [np.float32(0.25), np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf),
            finite[0], finite[1], np.float32(np.nextafter(np.float32(0.25), np.float32(1))), np.float32(-0.4)]
    for cut in cuts:
        for limit in (0, 1, 7, n, n + 50, -3):
            rows, sc, total = above_model.above(s, dead, cut, limit)
            erows, etotal = _brute(s, dead, cut, limit)
            assert total == etotal, (float(cut), limit)
            assert rows.tolist() == erows, (float(cut), limit)
            assert sc.view(np.uint32).tolist() == s[rows].view(np.uint32).tolist()


def test_cut_equal_to_a_score_includes_it_and_zero_signs_agree():
    s = np.array([0.5, 0.25, 0.25, -0.0, 0.0, -1.0], dtype=np.float32)
    rows, _, total = above_model.above(s, None, np.float32(0.25), 10)
    assert rows.tolist() == [0, 2, 1] and total == 3
    a = above_model.above(s, None, np.float32(0.0), 10)
    b = above_model.above(s, None, np.float32(-0.0), 10)
    assert a[0].tolist() == b[0].tolist() == [0, 2, 1, 4, 3] and a[2] == b[2] == 5


@pytest.mark.parametrize("seed", range(3))
def test_total_is_the_length_of_the_full_list(seed):
    rng = np.random.default_rng(100 + seed)
    s = _vector(rng, 300)
    dead = rng.random(300) < 0.1
    for cut in (np.float32(-np.inf), np.float32(-0.5), np.float32(0.25), np.float32(2.0)):
        rows, _, total = above_model.above(s, dead, cut, 300)
        assert len(rows) == total
        assert not dead[rows].any()
    assert above_model.above(s, dead, np.float32(-np.inf), 300)[2] == int((~dead).sum())


def test_cut_for_total():
    rng = np.random.default_rng(5)
    s = rng.standard_normal(500).astype(np.float32)
    dead = rng.random(500) < 0.2
    for t in (0, 1, 17, int((~dead).sum())):
        cut = above_model.cut_for_total(s, dead, t)
        assert above_model.above(s, dead, cut, 0)[2] == t

"""CPU: the numpy model of the scoped collapsed search (collapse_scope_model.py) against a plain Python dict group-by
over the definition, on hand-written cases and on small random inputs."""
import numpy as np

from collapse_scope_model import collapsed_scoped
from test_collapse_model import _bits, _key


def loop(scores, values, dead, in_scope, zero_single, k):
    """The definition, row by row: S = the live rows in scope; a dict from group to its best key over S."""
    best, matched = {}, 0
    for r in range(len(scores)):
        if not in_scope[r] or (dead is not None and dead[r]):
            continue
        matched += 1
        v = 0 if values is None else int(values[r])
        g = ("row", r) if zero_single and v == 0 else ("value", v)
        best[g] = max(best.get(g, 0), _key(scores[r], r))
    w = sorted(best.values(), reverse=True)
    rows = [key & 0xFFFFFFFF for key in w[:min(max(k, 0), len(w))]]
    return rows, [0 if values is None else int(values[r]) for r in rows], len(w), matched


def _agree(scores, values, dead, in_scope, zero_single, k):
    s, r, v, g, m = collapsed_scoped(scores, values, dead, in_scope, zero_single, k)
    rows, vals, groups, matched = loop(scores, values, dead, in_scope, zero_single, k)
    assert (r.tolist(), v.tolist(), g, m) == (rows, vals, groups, matched)
    assert _bits(s) == _bits(np.asarray(scores, dtype=np.float32)[rows])      # the bits of the score vector
    assert s.dtype == np.float32 and r.dtype == np.int64 and v.dtype == np.uint32
    return r.tolist(), v.tolist(), g, m


#         row:   0    1    2    3    4     5    6    7    8
S = np.array([0.5, 0.9, 0.1, 0.9, -0.2, 0.3, 0.9, 0.0, 0.4], dtype=np.float32)
V = np.array([7,   3,   7,   3,   0,    0,   5,   9,   0xFFFFFFFF], dtype=np.uint32)
ALL = np.ones(9, dtype=bool)


def test_hand_written():
    # the whole index in scope: collapse_model's answers, matched = 9
    assert _agree(S, V, None, ALL, True, 10) == ([6, 3, 0, 8, 5, 7, 4], [5, 3, 7, 0xFFFFFFFF, 0, 9, 0], 7, 9)
    assert _agree(S, V, None, ALL, False, 10) == ([6, 3, 0, 8, 5, 7], [5, 3, 7, 0xFFFFFFFF, 0, 9], 6, 9)
    # the odd rows: value 3 keeps its tie (row 3 over row 1), value 7 and 5 and 0xFFFFFFFF have no row in scope
    odd = np.arange(9) % 2 == 1
    assert _agree(S, V, None, odd, True, 10) == ([3, 5, 7], [3, 0, 9], 3, 4)
    # row 3 out of scope: the representative of value 3 is its best row IN scope, with that row's own score
    scope = ALL.copy()
    scope[3] = False
    r, v, g, m = _agree(S, V, None, scope, True, 10)
    assert r[:2] == [6, 1] and (g, m) == (7, 8)
    # out of scope and dead are one thing to the groups, and only live rows in scope count as matched
    dead = np.zeros(9, dtype=bool)
    dead[[1, 6]] = True
    assert _agree(S, V, dead, scope, True, 10) == ([0, 8, 5, 7, 4], [7, 0xFFFFFFFF, 0, 9, 0], 5, 6)
    # k cuts the list, not the counts; k <= 0 only counts
    assert _agree(S, V, None, odd, True, 2) == ([3, 5], [3, 0], 3, 4)
    for k in (0, -3):
        assert _agree(S, V, None, odd, True, k) == ([], [], 3, 4)


def test_empty_scopes():
    none = np.zeros(9, dtype=bool)
    for zero_single in (False, True):
        assert _agree(S, V, None, none, zero_single, 5) == ([], [], 0, 0)
        assert _agree(S, V, ALL, ALL, zero_single, 5) == ([], [], 0, 0)            # every row dead
    only_dead = np.zeros(9, dtype=bool)
    only_dead[[2, 4]] = True
    assert _agree(S, V, only_dead, only_dead, True, 5) == ([], [], 0, 0)           # the scope holds dead rows only
    assert _agree(np.zeros(0, dtype=np.float32), None, None, np.zeros(0, dtype=bool), True, 3) == ([], [], 0, 0)


def test_value_zero_and_a_column_never_set():
    scope = np.array([1, 0, 1, 0, 1, 1, 0, 1, 1], dtype=bool)
    # value 0 (rows 4, 5): two groups under zero_single, one -- its best row -- otherwise
    assert _agree(S, V, None, scope, True, 10) == ([0, 8, 5, 7, 4], [7, 0xFFFFFFFF, 0, 9, 0], 5, 6)
    assert _agree(S, V, None, scope, False, 10) == ([0, 8, 5, 7], [7, 0xFFFFFFFF, 0, 9], 4, 6)
    # identities (a) and (b): no column -> the plain top-k over S under zero_single, its first row otherwise
    order = sorted(np.flatnonzero(scope).tolist(), key=lambda r: _key(S[r], r), reverse=True)
    assert _agree(S, None, None, scope, True, 100) == (order, [0] * 6, 6, 6)
    assert _agree(S, None, None, scope, False, 100) == (order[:1], [0], 1, 6)


def test_key_space():
    # -0.0 and +0.0 tie: the larger row in scope wins
    s = np.array([0.0, -0.0, -0.0, 0.0, -1.0], dtype=np.float32)
    assert _agree(s, [4, 4, 6, 6, 4], None, np.ones(5, dtype=bool), False, 5) == ([3, 1], [6, 4], 2, 5)
    assert _agree(s, [4, 4, 6, 6, 4], None, np.array([1, 0, 1, 0, 1], dtype=bool), False, 5) == ([2, 0], [6, 4], 2, 3)
    # a NaN in scope is the largest; the same NaN out of scope is absent
    s = np.array([np.inf, np.nan, 0.5, -np.inf, 0.7, np.nan], dtype=np.float32)
    v = [1, 1, 2, 3, 2, 9]
    assert _agree(s, v, None, np.ones(6, dtype=bool), False, 5) == ([5, 1, 4, 3], [9, 1, 2, 3], 4, 6)
    assert _agree(s, v, None, np.array([1, 0, 1, 1, 1, 0], dtype=bool), False, 5) == ([0, 4, 3], [1, 2, 3], 3, 4)


def test_random_inputs_agree_with_the_loop():
    rng = np.random.default_rng(23)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.25, 0.25, 0.25], dtype=np.float32)
    for trial in range(200):
        n = int(rng.integers(1, 60))
        s = rng.standard_normal(n).astype(np.float32)
        put = rng.random(n) < 0.3                            # ties, NaN, zeros of both signs, infinities
        s[put] = rng.choice(special, int(put.sum()))
        pool = np.array([0, 0, 1, 2, 3, 1 << 22, 2 << 22, 0xFFFFFFFF, 77], dtype=np.uint32)
        v = rng.choice(pool[:int(rng.integers(1, len(pool) + 1))], n).astype(np.uint32)
        dead = rng.random(n) < (0.0, 0.2, 0.9)[trial % 3]
        scope = rng.random(n) < (0.0, 0.1, 0.5, 1.0)[trial % 4]   # empty, thin, half, everything
        for zero_single in (False, True):
            for k in (0, 1, 3, n, n + 5):
                _agree(s, v, dead if trial % 3 else None, scope, zero_single, k)
        _agree(s, None, dead, scope, bool(trial & 1), n)

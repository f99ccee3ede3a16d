"""CPU: the numpy model of the collapsed search (collapse_model.py) against a plain Python dict loop over the
definition, on hand-written cases and on small random inputs."""
import struct

import numpy as np

import collapse_model
from collapse_model import collapsed


def _key(x, r):
    """keys.h make_key in plain Python: (orderable score, row) as one integer."""
    u = struct.unpack("<I", struct.pack("<f", float(x)))[0]
    if (u & 0x7FFFFFFF) > 0x7F800000:
        k = 0xFFFFFFFF                       # NaN: the largest
    else:
        if u == 0x80000000:
            u = 0                            # -0.0 -> +0.0
        k = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (k << 32) | r


def loop(scores, values, dead, zero_single, k):
    """The definition, row by row: a dict from group to its best key."""
    best = {}
    for r in range(len(scores)):
        if dead is not None and dead[r]:
            continue
        v = 0 if values is None else int(values[r])
        g = ("row", r) if zero_single and v == 0 else ("value", v)
        key = _key(scores[r], r)
        if g not in best or key > best[g]:
            best[g] = key
    w = sorted(best.values(), reverse=True)
    rows = [key & 0xFFFFFFFF for key in w[:min(max(k, 0), len(w))]]
    return rows, [0 if values is None else int(values[r]) for r in rows], len(w)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).tolist()


def _agree(scores, values, dead, zero_single, k):
    s, r, v, g = collapsed(scores, values, dead, zero_single, k)
    rows, vals, groups = loop(scores, values, dead, zero_single, k)
    assert (r.tolist(), v.tolist(), g) == (rows, vals, groups)
    assert _bits(s) == _bits(np.asarray(scores, dtype=np.float32)[rows])      # the bits of the score vector
    assert s.dtype == np.float32 and r.dtype == np.int64 and v.dtype == np.uint32
    return r.tolist(), v.tolist(), g


#         row:   0    1    2    3    4     5    6    7    8
S = np.array([0.5, 0.9, 0.1, 0.9, -0.2, 0.3, 0.9, 0.0, 0.4], dtype=np.float32)
V = np.array([7,   3,   7,   3,   0,    0,   5,   9,   0xFFFFFFFF], dtype=np.uint32)


def test_hand_written():
    # value 5: row 6 (0.9); value 3: rows 1, 3 (0.9 twice: row 3 wins); 7: rows 0, 2; 9: row 7; 0xFFFFFFFF: row 8; 0: rows 4, 5
    assert _agree(S, V, None, True, 10) == ([6, 3, 0, 8, 5, 7, 4], [5, 3, 7, 0xFFFFFFFF, 0, 9, 0], 7)
    assert _agree(S, V, None, False, 10) == ([6, 3, 0, 8, 5, 7], [5, 3, 7, 0xFFFFFFFF, 0, 9], 6)
    # k cuts the list, not the group count; k <= 0 only counts
    assert _agree(S, V, None, True, 2) == ([6, 3], [5, 3], 7)
    for k in (0, -3):
        assert _agree(S, V, None, True, k) == ([], [], 7)
    # no column: the plain top-k under zero_single, the best live row otherwise
    order = sorted(range(9), key=lambda r: _key(S[r], r), reverse=True)
    assert _agree(S, None, None, True, 100) == (order, [0] * 9, 9)
    assert _agree(S, None, None, False, 100) == ([6], [0], 1)
    assert _agree(np.zeros(0, dtype=np.float32), None, None, True, 3) == ([], [], 0)


def test_dead_rows():
    dead = np.zeros(9, dtype=bool)
    dead[3] = True                                           # the best row of value 3: the runner-up takes over
    r, v, g = _agree(S, V, dead, True, 10)
    assert r[:2] == [6, 1] and g == 7
    dead[1] = True                                           # every row of value 3: the group is gone
    r, v, g = _agree(S, V, dead, True, 10)
    assert 3 not in v and g == 6
    dead[[4, 5]] = True                                      # exempt rows die one by one; value 0 as a group dies whole
    assert _agree(S, V, dead, True, 10)[2] == 4 and _agree(S, V, dead, False, 10)[2] == 4
    assert _agree(S, V, np.ones(9, dtype=bool), True, 10) == ([], [], 0)


def test_key_space():
    # -0.0 and +0.0 tie: the larger row wins inside a group, and comes first across groups
    s = np.array([0.0, -0.0, -0.0, 0.0, -1.0], dtype=np.float32)
    assert _agree(s, [4, 4, 6, 6, 4], None, False, 5) == ([3, 1], [6, 4], 2)
    # a NaN is the largest; -inf the smallest but still a row of W; +inf below a NaN
    s = np.array([np.inf, np.nan, 0.5, -np.inf, 0.7, np.nan], dtype=np.float32)
    assert _agree(s, [1, 1, 2, 3, 2, 9], None, False, 5) == ([5, 1, 4, 3], [9, 1, 2, 3], 4)
    sc = collapsed(s, [1, 1, 2, 3, 2, 9], None, False, 5)[0]
    assert np.isnan(sc[0]) and np.isnan(sc[1]) and sc[3] == -np.inf


def test_random_inputs_agree_with_the_loop():
    rng = np.random.default_rng(11)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 0.25, 0.25, 0.25], dtype=np.float32)
    for trial in range(200):
        n = int(rng.integers(1, 60))
        s = rng.standard_normal(n).astype(np.float32)
        put = rng.random(n) < 0.3                            # ties, NaN, zeros of both signs, infinities
        s[put] = rng.choice(special, int(put.sum()))
        pool = np.array([0, 0, 1, 2, 3, 1 << 22, 2 << 22, 0xFFFFFFFF, 77], dtype=np.uint32)
        v = rng.choice(pool[:int(rng.integers(1, len(pool) + 1))], n).astype(np.uint32)
        dead = rng.random(n) < (0.0, 0.2, 0.9)[trial % 3]    # none, some, nearly all: groups whose rows are all dead
        for zero_single in (False, True):
            for k in (0, 1, 3, n, n + 5):
                _agree(s, v, dead if trial % 3 else None, zero_single, k)
        _agree(s, None, dead, bool(trial & 1), n)


def test_score_key_is_above_models():
    import above_model
    assert collapse_model.score_key is above_model.score_key

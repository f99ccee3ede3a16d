"""CPU: the f64 model of the diverse (MMR) search and its validity check (tests/diverse_model.py) -- the check must
accept the model's own answer and reject the answers a broken kernel would give."""
import numpy as np
import pytest

import diverse_model as dm

D = 16


def _case(seed=5, n=600, c=32):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, D))
    m = (m / np.linalg.norm(m, axis=1, keepdims=True)).astype(np.float32)
    q = rng.standard_normal(D)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    sc = m.astype(np.float64) @ q.astype(np.float64)
    order = np.argsort(-sc, kind="stable")[:c]
    return sc[order].astype(np.float32), m[order]


def test_model_accepts_its_own_picks():
    s, R = _case()
    for lam in (0.3, 0.5, 0.9):
        picks, red = dm.greedy(s, dm.gram64(R), 10, lam)
        assert len(set(picks)) == 10 and picks[0] == 0 and red[0] == -np.inf
        assert dm.valid_picks(s, R, picks, np.array(red, dtype=np.float32), lam, D) == 0
    # lam = 1: relevance alone, the candidates in order
    picks, _ = dm.greedy(s, dm.gram64(R), 10, 1.0)
    assert picks == list(range(10))
    # k past the candidates: all of them, once each
    picks, _ = dm.greedy(s, dm.gram64(R), 100, 0.5)
    assert sorted(picks) == list(range(len(s)))


def test_model_rejects_plain_top_k():
    s, R = _case()
    G = dm.gram64(R)
    picks, _ = dm.greedy(s, G, 10, 0.5)
    assert picks != list(range(10))
    plain = list(range(10))
    red = [-np.inf] + [float(G[p, plain[:t]].max()) for t, p in enumerate(plain) if t]
    with pytest.raises(AssertionError, match="objective"):
        dm.valid_picks(s, R, plain, red, 0.5, D)


def test_model_rejects_swapped_picks():
    s, R = _case()
    G = dm.gram64(R)
    picks, red = dm.greedy(s, G, 10, 0.5)
    swapped = list(picks)
    swapped[1], swapped[2] = swapped[2], swapped[1]
    red2 = [-np.inf] + [float(G[p, swapped[:t]].max()) for t, p in enumerate(swapped) if t]
    with pytest.raises(AssertionError, match="step 1"):
        dm.valid_picks(s, R, swapped, red2, 0.5, D)


def test_model_rejects_repeated_pick_and_wrong_redundancy():
    s, R = _case()
    picks, red = dm.greedy(s, dm.gram64(R), 10, 0.5)
    twice = list(picks)
    twice[7] = twice[3]
    with pytest.raises(AssertionError, match="twice"):
        dm.valid_picks(s, R, twice, red, 0.5, D)
    off = list(red)
    off[4] += 1e-4
    with pytest.raises(AssertionError, match="redundancy"):
        dm.valid_picks(s, R, picks, off, 0.5, D)
    with pytest.raises(AssertionError, match="best candidate"):
        dm.valid_picks(s, R, picks[1:], red[1:], 0.5, D)


def test_tolerance_at_the_gpu_test_shape():
    R = np.zeros((2, 64))
    R[:, 0] = 1.0
    e_g, tol = dm.tolerances(R, 0.0, 64)
    assert abs(e_g - 66 * 2.0 ** -24) < 1e-15 and 8.2e-6 < tol < 8.4e-6

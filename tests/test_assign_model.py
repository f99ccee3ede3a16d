"""CPU: the f64 model of the nearest-vector assignment and its validity check (tests/assign_model.py) -- the check must
accept the model's own answer and reject the answers a broken kernel would give."""
import numpy as np
import pytest

import assign_model as am

D = 16


def _unit(rng, n, d=D):
    v = rng.standard_normal((n, d))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _case(seed=7, n=500, c=9):
    rng = np.random.default_rng(seed)
    return _unit(rng, n), _unit(rng, c)


def test_model_accepts_its_own_answer():
    R, V = _case()
    best, score, counts = am.assign64(R, V)
    assert counts.sum() == len(R) and len(set(best.tolist())) > 1
    assert am.valid_assignment(R, V, best, score.astype(np.float32), counts) == 0
    # without scores, without counts
    assert am.valid_assignment(R, V, best, None, None) == 0
    # tombstones leave the counts only
    live = np.ones(len(R), dtype=bool)
    live[::7] = False
    b2, s2, c2 = am.assign64(R, V, live)
    assert np.array_equal(b2, best) and c2.sum() == live.sum()
    assert am.valid_assignment(R, V, b2, s2, c2, live) == 0
    with pytest.raises(AssertionError, match="bincount"):
        am.valid_assignment(R, V, b2, s2, counts, live)


def test_model_breaks_ties_to_the_lower_position():
    R, V = _case()
    V = np.concatenate([V, V[2:3]])          # position 9 is a copy of position 2
    best, _, counts = am.assign64(R, V)
    assert (best != 9).all() and counts[9] == 0 and counts[2] > 0
    # ... and the check cannot tell the copy from the original: those rows are reported as near ties
    swapped = np.where(best == 2, 9, best)
    near = am.valid_assignment(R, V, swapped, None, None)
    assert near >= counts[2]


def test_model_rejects_a_wrong_position_with_margin():
    R, V = _case()
    best, score, counts = am.assign64(R, V)
    _, tol = am.tolerances(R, V, D)
    r = int(np.argmax(am.margins(R, V)))
    assert am.margins(R, V)[r] > 100 * tol
    wrong = best.copy()
    wrong[r] = (best[r] + 1) % len(V)
    with pytest.raises(AssertionError, match=f"row {r}: assigned"):
        am.valid_assignment(R, V, wrong, None, None)
    # a kernel that ignores the data
    with pytest.raises(AssertionError, match="assigned"):
        am.valid_assignment(R, V, np.zeros(len(R), dtype=np.int32), None, None)
    # a position outside the vectors
    out = best.copy()
    out[3] = len(V)
    with pytest.raises(AssertionError, match="outside"):
        am.valid_assignment(R, V, out, None, None)


def test_model_rejects_wrong_scores_and_counts():
    R, V = _case()
    best, score, counts = am.assign64(R, V)
    off = score.copy()
    off[11] += 1e-4
    with pytest.raises(AssertionError, match="row 11: score"):
        am.valid_assignment(R, V, best, off, counts)
    nan = score.copy()
    nan[5] = np.nan
    with pytest.raises(AssertionError, match="row 5: score"):
        am.valid_assignment(R, V, best, nan, counts)
    c2 = counts.copy()
    c2[0] += 1
    with pytest.raises(AssertionError, match="bincount"):
        am.valid_assignment(R, V, best, score, c2)


def test_a_near_tie_is_accepted_either_way_and_counted():
    R, V = _case(c=4)
    _, tol = am.tolerances(R, V, D)
    V = V.astype(np.float64)
    V = np.concatenate([V, V[1:2] * (1.0 - 1e-9)])     # position 4: position 1 scaled down by less than tol
    best, _, _ = am.assign64(R, V)
    hit = np.flatnonzero(best == 1)
    assert hit.size
    other = best.copy()
    other[hit] = 4
    assert am.valid_assignment(R, V, other, None, None) >= hit.size


def test_single_vector():
    R, V = _case(c=1)
    best, score, counts = am.assign64(R, V)
    assert (best == 0).all() and counts.tolist() == [len(R)] and np.isinf(am.margins(R, V)).all()
    assert am.valid_assignment(R, V, best, score, counts) == 0


def test_tolerance_at_the_gpu_test_shape():
    R = np.zeros((2, 64))
    R[:, 0] = 1.0
    V = np.zeros((3, 64))
    V[:, 1] = 2.0
    e_a, tol = am.tolerances(R, V, 64)
    assert abs(e_a - 2 * 66 * 2.0 ** -24) < 1e-15 and tol == 2 * e_a

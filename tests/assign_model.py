"""The model of svs_index_assign (nearest-vector assignment), in f64, and the check a device result must pass.  Not a
test module: tests/test_assign_model.py tests it on the CPU, the GPU and host tests use it.

Definition (include/svs_amd.h): S = R V^T over the STORED rows R and the STORED vectors V (fp8: dequantised -- what
``stored_rows`` / ``stored_query`` return); best[r] = arg max_j S[r][j], an exact tie going to the lower j;
counts[j] = the live rows with best == j.

The device accumulates S in f32, so a device answer is checked with derived tolerances, not compared position by
position:
    e_A = (d + 2) 2^-24 max ||row|| max ||vector||    the f32 accumulation bound gamma_d sum |a b| <= gamma_d ||a|| ||b||
                                                      (Cauchy-Schwarz on two different operands: the bound
                                                      diverse_model.tolerances derives), plus two roundings for the
                                                      fp8 scales
    tol = 2 e_A                                       each side of a comparison its own error
At d = 64 on unit rows and unit vectors e_A = 3.9e-6 and tol = 7.9e-6.
"""
import numpy as np

EPS = 2.0 ** -24


def scores64(R, V):
    return np.asarray(R, dtype=np.float64) @ np.asarray(V, dtype=np.float64).T


def tolerances(R, V, d):
    """(e_A, tol) for the stored rows R and the stored vectors V."""
    R = np.asarray(R, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    e_a = (d + 2) * EPS * float(np.sqrt((R * R).sum(axis=1).max())) * float(np.sqrt((V * V).sum(axis=1).max()))
    return e_a, 2.0 * e_a


def assign64(R, V, live=None):
    """The f64 answer: (best i32, score f64, counts i64); ``live``: a boolean per row (None: every row)."""
    S = scores64(R, V)
    best = np.argmax(S, axis=1).astype(np.int32)          # (argmax returns the FIRST maximum: the lower position)
    sel = best if live is None else best[np.asarray(live, dtype=bool)]
    return best, S[np.arange(len(best)), best], np.bincount(sel, minlength=S.shape[1]).astype(np.int64)


def margins(R, V):
    """Per row, the f64 gap between the best and the second best score (+inf with one vector)."""
    S = scores64(R, V)
    if S.shape[1] < 2:
        return np.full(S.shape[0], np.inf)
    top = np.partition(S, S.shape[1] - 2, axis=1)
    return top[:, -1] - top[:, -2]


def valid_assignment(R, V, best, score, counts, live=None, d=None):
    """Asserts that (best, score, counts) is a valid answer for the stored rows R (the range's, in order) and the stored
    vectors V; ``score`` may be None.  Returns the number of rows on which a second position lies within ``tol`` of the
    best: there the check cannot tell two answers apart."""
    R = np.asarray(R, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    n, c = R.shape[0], V.shape[0]
    d = R.shape[1] if d is None else d
    best = np.asarray(best)
    assert best.shape == (n,), f"best has shape {best.shape} for {n} rows"
    assert ((best >= 0) & (best < c)).all(), "a position outside the vectors"
    S = scores64(R, V)
    e_a, tol = tolerances(R, V, d)
    top = S.max(axis=1)
    mine = S[np.arange(n), best]
    bad = np.flatnonzero(~(mine >= top - tol))
    assert bad.size == 0, (f"row {bad[0]}: assigned to {best[bad[0]]} with score {mine[bad[0]]!r}, the best is "
                           f"{int(np.argmax(S[bad[0]]))} with {top[bad[0]]!r} (tol {tol:.3g}); {bad.size} such rows")
    if score is not None:
        score = np.asarray(score, dtype=np.float64)
        assert score.shape == (n,)
        off = np.flatnonzero(~(np.abs(score - mine) <= e_a))
        assert off.size == 0, f"row {off[0]}: score {score[off[0]]!r}, f64 says {mine[off[0]]!r} (e_A {e_a:.3g}); {off.size} such rows"
    if counts is not None:
        sel = best if live is None else best[np.asarray(live, dtype=bool)]
        want = np.bincount(sel, minlength=c)
        assert np.array_equal(np.asarray(counts, dtype=np.int64), want), "the counts are not the bincount of best over the live rows"
    return int(((S >= (top - tol)[:, None]).sum(axis=1) >= 2).sum())

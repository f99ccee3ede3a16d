"""The model of svs_index_search_diverse (maximal marginal relevance over a search's candidates), in f64, and the
check a device result must pass.  Not a test module: tests/test_diverse_model.py tests it on the CPU, the GPU and host
tests use it.

Definition (include/svs_amd.h): candidates 0 .. c-1 in the search's order with scores s; G = R R^T over the STORED
candidate rows R; pick 0 is position 0; pick t >= 1 is the unpicked p with the largest
    obj(p) = lam * s[p] - (1 - lam) * red[p],     red[p] = max over earlier picks j of G[p][j],
an exact tie going to the lower position.  lam and 1 - lam are the f32 values the library computes with.

The device accumulates G in f32, so a device result is checked with derived tolerances, not compared pick by pick:
    e_G = (d + 2) 2^-24 max ||row||^2     the f32 accumulation bound gamma_d sum |a b| <= gamma_d ||a|| ||b||
                                          (Cauchy-Schwarz), plus two roundings for the fp8 scales
    tol = 2 ((1 - lam) e_G + 4 2^-24)     each side of a comparison its error in G and four roundings of the objective
At d = 64 on unit rows e_G = 3.9e-6 and tol <= 8.3e-6.
"""
import numpy as np

EPS = 2.0 ** -24


def lam_pair(lam):
    """(lambda_mult, 1 - lambda_mult) as the library holds them: f32 values, returned as Python floats."""
    l32 = np.float32(lam)
    return float(l32), float(np.float32(1.0) - l32)


def tolerances(R, lam, d):
    """(e_G, tol) for the stored candidate rows R."""
    R = np.asarray(R, dtype=np.float64)
    e_g = (d + 2) * EPS * float((R * R).sum(axis=1).max())
    return e_g, 2.0 * (lam_pair(lam)[1] * e_g + 4.0 * EPS)


def gram64(R):
    R = np.asarray(R, dtype=np.float64)
    return R @ R.T


def greedy(s, G, k, lam):
    """The f64 greedy: (picks, red) with red[t] the redundancy of pick t when it was chosen (-inf for pick 0)."""
    s = np.asarray(s, dtype=np.float64)
    c = len(s)
    count = min(max(k, 0), c)
    l, oml = lam_pair(lam)
    picks, reds = [], []
    red = np.full(c, -np.inf)
    free = np.ones(c, dtype=bool)
    for t in range(count):
        if t == 0:
            p = 0
        else:
            red = np.maximum(red, G[:, picks[-1]])
            obj = np.where(free, l * s - oml * red, -np.inf)
            p = int(np.argmax(obj))          # (argmax returns the FIRST maximum: the lower position)
        picks.append(p)
        reds.append(float(red[p]))
        free[p] = False
    return picks, reds


def valid_picks(s, R, picks, red_dev, lam, d):
    """Asserts that ``picks`` (candidate positions in pick order) with the reported redundancies ``red_dev`` is a valid
    answer for candidate scores ``s`` (the device's) and stored candidate rows ``R``; returns the number of steps at
    which a second candidate lay within ``tol`` of the best (there the check cannot tell two answers apart).
    red64 follows the DEVICE's own earlier picks, so the check stays sound after a legitimate near-tie, and wherever the
    margin exceeds tol it forces the f64 arg-max exactly."""
    s = np.asarray(s, dtype=np.float64)
    c = len(s)
    picks = [int(p) for p in picks]
    red_dev = np.asarray(red_dev, dtype=np.float64)
    assert len(picks) == len(red_dev) and 1 <= len(picks) <= c
    assert all(0 <= p < c for p in picks), "a pick outside the candidate list"
    assert len(set(picks)) == len(picks), "a candidate was picked twice"
    assert picks[0] == 0, "pick 0 must be the best candidate"
    assert red_dev[0] == -np.inf, "the first pick's redundancy is the max over nothing"
    G = gram64(R)
    e_g, tol = tolerances(R, lam, d)
    l, oml = lam_pair(lam)
    red = np.full(c, -np.inf)
    free = np.ones(c, dtype=bool)
    free[0] = False
    near = 0
    for t in range(1, len(picks)):
        red = np.maximum(red, G[:, picks[t - 1]])
        obj = l * s - oml * red
        best = obj[free].max()
        p = picks[t]
        assert obj[p] >= best - tol, f"step {t}: picked position {p} with objective {obj[p]!r}, the best is {best!r} (tol {tol:.3g})"
        assert abs(red_dev[t] - red[p]) <= e_g, f"step {t}: redundancy {red_dev[t]!r}, f64 says {red[p]!r} (e_G {e_g:.3g})"
        if int((obj[free] >= best - tol).sum()) >= 2:
            near += 1
        free[p] = False
    return near

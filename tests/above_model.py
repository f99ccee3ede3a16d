"""The definition of the threshold search (svs_index_search_above) in numpy: shared by the CPU and the GPU tests.

``score_key`` is keys.h's orderable key on uint32 views (-0.0 folded onto +0.0, any NaN mapped to the maximum); row r
qualifies iff it is live and ``score_key(s[r]) >= score_key(cut)``; the answer lists the qualifying rows by
(key desc, row desc)."""
import numpy as np


def score_key(x) -> np.ndarray:
    """keys.h score_key: f32 -> u32 whose unsigned order is the order of the search results."""
    u = np.atleast_1d(np.asarray(x, dtype=np.float32)).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0                                  # -0.0 -> +0.0
    neg = (u & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = np.uint32(0xFFFFFFFF)
    return k


def above(scores, dead, cut, limit):
    """(rows i64 (count,), scores f32 (count,), total): the first min(max(limit, 0), total) rows of
    A = {live r : score_key(scores[r]) >= score_key(cut)} by (key desc, row desc); scores are the bits of ``scores``."""
    s = np.asarray(scores, dtype=np.float32)
    key = score_key(s)
    live = np.ones(len(s), dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
    rows = np.nonzero(live & (key >= score_key(cut)[0]))[0].astype(np.int64)
    total = len(rows)
    full = (key[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    order = np.argsort(full, kind="stable")[::-1][:min(max(int(limit), 0), total)]
    rows = rows[order]
    return rows, s[rows], total


def cut_for_total(scores, dead, t):
    """A cut-off under which exactly the t best live rows qualify: the t-th best live score (whose key must differ from the
    (t+1)-th's); t == 0: above the maximum (+inf; needs no NaN / +inf score among the live rows)."""
    s = np.asarray(scores, dtype=np.float32)
    live = np.ones(len(s), dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
    if t == 0:
        assert (score_key(s[live]) < score_key(np.inf)[0]).all()
        return np.float32(np.inf)
    k = np.sort(score_key(s[live]))[::-1]
    assert t <= len(k) and (t == len(k) or k[t] < k[t - 1]), "the t-th and (t+1)-th best scores tie"
    live_rows = np.nonzero(live)[0]
    kk = score_key(s[live_rows])
    return s[live_rows[np.nonzero(kk == k[t - 1])[0][0]]]

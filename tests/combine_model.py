"""The numpy model of a combined search (svs_index_search_combined; include/svs_amd.h, svs_amd/csrc/combine.h), written
from the definition and not from kernel output.

Given the m score vectors s_j (what ``idx.scores(v_j)`` returns), f32 weights and an op:
    t_j = w_j * s_j                      one np.float32 multiplication (weights None: t_j = s_j)
    max / min   key_score(max_j / min_j score_key(t_j))       the order's key: -0 folds onto +0, any NaN is the largest
    sum         ((t_0 + t_1) + t_2) + ...                     np.float32 additions in vector order
The top-k is select_model.expected_scores of that vector with the tombstoned rows at -inf.
"""
from __future__ import annotations

import numpy as np

import select_model

OPS = ("max", "min", "sum")


def terms(scores, weights=None):
    """[t_j] as f32 arrays."""
    s = [np.asarray(v, dtype=np.float32) for v in scores]
    if weights is None:
        return s
    w = np.asarray(weights, dtype=np.float32)
    assert w.shape == (len(s),)
    with np.errstate(all="ignore"):
        return [(w[j] * s[j]).astype(np.float32) for j in range(len(s))]


def combine(scores, weights=None, op: str = "max") -> np.ndarray:
    """The combined f32 vector of all rows."""
    t = terms(scores, weights)
    assert len(t) >= 1 and op in OPS
    if op == "sum":
        acc = t[0].copy()
        with np.errstate(all="ignore"):
            for x in t[1:]:
                acc = (acc + x).astype(np.float32)
        return acc
    keys = np.stack([select_model.score_key(x) for x in t])
    return select_model.key_score(keys.max(axis=0) if op == "max" else keys.min(axis=0))


def top_k(scores, weights, op: str, k: int, dead=None, row_offset: int = 0):
    """(score bits u32[k], rows i64[k], count): run_select over the combined vector with the rows `dead` masked."""
    c = combine(scores, weights, op).copy()
    dead = np.zeros(0, dtype=np.int64) if dead is None else np.asarray(dead, dtype=np.int64)
    c[dead] = -np.inf
    count = min(max(int(k), 0), c.size - dead.size)
    bits, rows = select_model.expected_scores(c, count, row_offset)
    out_b = np.full(k, np.float32(-np.inf).view(np.uint32), dtype=np.uint32)
    out_r = np.full(k, -1, dtype=np.int64)
    out_b[:count], out_r[:count] = bits, rows
    return out_b, out_r, count

"""The definition of the group-combined search (svs_index_search_collapsed_combined; include/svs_amd.h) in numpy,
written from the definition and not from kernel output: shared by the CPU and the GPU tests.

Given the m score vectors s_j (what ``idx.scores(v_j)`` returns), f32 weights, an op, the column and the dead rows:
    groups      collapse_model's: a row's value, or -- value 0 under ``zero_single`` -- the row itself
    M_j(G)      max over the live rows of G of score_key(s_j[r])          (above_model.score_key: keys.h's key)
    c(G)        combine_model.combine over the m one-element vectors key_score(M_j(G)), the weights and the op
    c_row       combine_model.combine over the s_j themselves: the row-level combined vector
    rep(G)      the live row of G with the largest score_key(c_row[r]) << 32 | r
and the answer lists the groups by score_key(c(G)) << 32 | rep(G), descending.  Scores come back as every search
returns them: key_score(score_key(c)), that is -0.0 as +0.0 and any NaN as 0x7fc00000."""
import numpy as np

import combine_model
import select_model
from above_model import score_key


def _group_ids(v, rows, zero_single):
    """One u64 per live row: its value, or -- an exempt row -- a number no value can be, different for every row."""
    group = v[rows].astype(np.uint64)
    if zero_single:
        alone = v[rows] == 0
        group[alone] = (np.uint64(1) << np.uint64(32)) + rows[alone].astype(np.uint64)
    return group


def collapsed_combined(scores, weights, op, values, dead, zero_single, k):
    """(scores f32 (count,), rows i64 (count,), values u32 (count,), groups): groups = the groups with a live row,
    count = min(max(k, 0), groups).  ``scores``: the m vectors; ``weights`` None: 1.0 each; ``values`` None: every row
    carries 0; ``dead`` None: every row is live (else a bool mask).  Rows are local."""
    s = [np.asarray(x, dtype=np.float32) for x in scores]
    m, n = len(s), len(s[0])
    v = np.zeros(n, dtype=np.uint32) if values is None else np.asarray(values, dtype=np.uint32)
    live = np.ones(n, dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
    rows = np.nonzero(live)[0]
    if len(rows) == 0:
        return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32), 0
    c_row = combine_model.combine(s, weights, op)
    full = (score_key(c_row)[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)   # make_key(c_row, r): unique
    group = _group_ids(v, rows, zero_single)
    order = np.lexsort((full, group))                                        # by group, then by key ascending
    rows, full, group = rows[order], full[order], group[order]
    first = np.nonzero(np.append(True, group[1:] != group[:-1]))[0]
    last = np.append(first[1:], len(rows)) - 1
    rep = rows[last]                                                         # a group's largest key: rep(G)
    best = [select_model.key_score(np.maximum.reduceat(score_key(s[j])[rows], first)) for j in range(m)]   # key_score(M_j(G))
    c = combine_model.combine(best, weights, op)                             # c(G), one per group
    gkey = (score_key(c).astype(np.uint64) << np.uint64(32)) | rep.astype(np.uint64)
    rank = np.argsort(gkey, kind="stable")[::-1][:min(max(int(k), 0), len(rep))]
    out = select_model.key_score(score_key(c[rank])).astype(np.float32)
    return out, rep[rank].astype(np.int64), v[rep[rank]], len(rep)


def brute_force(scores, weights, op, values, dead, zero_single, k):
    """The same answer by a Python loop over the rows, one group at a time, in plain Python floats and ints where the
    definition allows (keys are integers; the f32 chain is np.float32 arithmetic, one operation at a time)."""
    s = [np.asarray(x, dtype=np.float32) for x in scores]
    m, n = len(s), len(s[0])
    w = [np.float32(1.0)] * m if weights is None else [np.float32(x) for x in weights]

    def key(x):
        return int(score_key(np.array([x], dtype=np.float32))[0])

    def unkey(kk):
        return np.float32(select_model.key_score(np.array([kk], dtype=np.uint32))[0])

    def fold(xs):
        with np.errstate(all="ignore"):
            t = [np.float32(w[j] * xs[j]) for j in range(m)]
            if op == "sum":
                acc = np.float32(-0.0)
                for x in t:
                    acc = np.float32(acc + x)
                return acc
            ks = [key(x) for x in t]
            return unkey(max(ks) if op == "max" else min(ks))

    groups = {}
    for r in range(n):
        if dead is not None and dead[r]:
            continue
        val = 0 if values is None else int(values[r])
        g = ("row", r) if (zero_single and val == 0) else ("value", val)
        mj, rep = groups.get(g, ([0] * m, (-1, -1)))
        mj = [max(mj[j], key(s[j][r])) for j in range(m)]
        rep = max(rep, (key(fold([s[j][r] for j in range(m)])), r))
        groups[g] = (mj, rep)
    ranked = []
    for mj, (_, r) in groups.values():
        c = fold([unkey(x) for x in mj])
        ranked.append((key(c), r))
    ranked.sort(reverse=True)
    ranked = ranked[:min(max(int(k), 0), len(ranked))]
    out_s = np.array([unkey(kk) for kk, _ in ranked], dtype=np.float32)
    out_r = np.array([r for _, r in ranked], dtype=np.int64)
    out_v = np.array([0 if values is None else int(values[r]) for _, r in ranked], dtype=np.uint32)
    return out_s, out_r, out_v, len(groups)

"""The definition of the collapsed search (svs_index_search_collapsed) in numpy: shared by the CPU and the GPU tests.

Row r's group is its value ``v[r]``; with ``zero_single`` a row whose value is 0 is a group of its own.  best(G) = the
largest ``score_key(s[r]) << 32 | r`` over the LIVE rows of G (above_model.score_key: keys.h's orderable key, so -0.0
folds onto +0.0, a NaN is the largest and a score tie goes to the larger row); W = the rows that are the best of their
group; the answer lists W by key descending."""
import numpy as np

from above_model import score_key


def collapsed(scores, values, dead, zero_single, k):
    """(scores f32 (count,), rows i64 (count,), values u32 (count,), groups): groups = |W|, count = min(max(k, 0),
    groups).  ``values`` None: every row carries 0; ``dead`` None: every row is live.  Scores are the bits of
    ``scores``; rows are local."""
    s = np.asarray(scores, dtype=np.float32)
    n = len(s)
    v = np.zeros(n, dtype=np.uint32) if values is None else np.asarray(values, dtype=np.uint32)
    live = np.ones(n, dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
    rows = np.nonzero(live)[0]
    full = (score_key(s)[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)   # make_key: unique
    # the group of a row as one u64: its value, or -- an exempt row -- a number no value can be, different for every row
    group = v[rows].astype(np.uint64)
    if zero_single:
        alone = v[rows] == 0
        group[alone] = (np.uint64(1) << np.uint64(32)) + rows[alone].astype(np.uint64)
    order = np.lexsort((full, group))                                        # by group, then by key ascending
    rows, full, group = rows[order], full[order], group[order]
    last = np.nonzero(np.append(group[1:] != group[:-1], True))[0] if len(rows) else np.zeros(0, dtype=np.int64)
    w, wkey = rows[last], full[last]                                         # a group's largest key: best(G)
    rank = np.argsort(wkey, kind="stable")[::-1][:min(max(int(k), 0), len(w))]
    best = w[rank].astype(np.int64)
    return s[best], best, v[best], len(w)

"""The definition of the per-label breakdown (svs_index_search_by_label) in numpy: shared by the CPU and the GPU tests.

Row r belongs to A_l iff it is live, its label is l, and ``score_key(s[r]) >= score_key(cut)`` (above_model.score_key:
keys.h's orderable key).  G = the labels of the set whose A_l is not empty; best(l) = the largest
``score_key(s[r]) << 32 | r`` over A_l; the answer lists G by best(l) descending."""
import numpy as np

from above_model import score_key


def by_label(scores, labels, dead, label_set, cut, k):
    """(labels u32 (count,), scores f32 (count,), rows i64 (count,), totals i64 (count,), groups): count =
    min(max(k, 0), groups).  ``labels`` None: every row carries 0; ``dead`` None: every row is live; ``cut`` None: -inf;
    ``label_set``: any order, repeats allowed.  Scores are the bits of ``scores``; rows are local."""
    s = np.asarray(scores, dtype=np.float32)
    n = len(s)
    lab = np.zeros(n, dtype=np.uint32) if labels is None else np.asarray(labels, dtype=np.uint32)
    live = np.ones(n, dtype=bool) if dead is None else ~np.asarray(dead, dtype=bool)
    key = score_key(s)
    t = score_key(-np.inf if cut is None else cut)[0]
    wanted = np.array(sorted({int(x) for x in np.asarray(label_set).reshape(-1).tolist()}), dtype=np.uint32)
    rows = np.nonzero(live & (key >= t) & np.isin(lab, wanted))[0]           # the union of the A_l
    full = (key[rows].astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)   # make_key: unique
    order = np.lexsort((full, lab[rows]))                                    # by label, then by key ascending
    rows, full = rows[order], full[order]
    found, first, totals = np.unique(lab[rows], return_index=True, return_counts=True)   # G, and |A_l|
    last = first + totals - 1                                                # a label's largest key: best(l)
    rank = np.argsort(full[last], kind="stable")[::-1][:min(max(int(k), 0), len(found))]
    best = rows[last[rank]].astype(np.int64)
    return found[rank].astype(np.uint32), s[best], best, totals[rank].astype(np.int64), len(found)

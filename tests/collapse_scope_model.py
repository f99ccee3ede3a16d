"""The definition of the scoped collapsed search (svs_index_search_collapsed_where / _rows) in numpy: shared by the
CPU and the GPU tests.

The scope S is the live rows the predicate or the row list admits.  Everything else is collapse_model's definition with
the rows outside S treated like dead rows: a group is represented by its best row IN S, and a group with no row in S
has no representative.  ``t_full`` carries a score for every row; only the entries of S are read."""
import numpy as np

import collapse_model


def collapsed_scoped(t_full, values, dead, in_scope, zero_single, k):
    """(scores f32 (count,), rows i64 (count,), values u32 (count,), groups, matched): collapse_model.collapsed over
    the rows that are live and in scope, and matched = how many those are.  ``dead`` None: every row is live;
    ``in_scope``: bool (n,)."""
    scope = np.asarray(in_scope, dtype=bool)
    out = scope.copy() if dead is None else scope & ~np.asarray(dead, dtype=bool)
    s, r, v, groups = collapse_model.collapsed(t_full, values, ~out, zero_single, k)
    return s, r, v, groups, int(out.sum())

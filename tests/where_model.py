"""The numpy model of a ``where`` list (svs_index_search_where's predicate): terms ``(column, op, arg)``, all of which
must hold.  Plain definitions, written independently of svs_amd.index's packing: nothing here imports the product."""
import numpy as np

OPS = ("in", "not in", "range", "not range", "any_bits", "no_bits", "all_bits", "not all_bits")


def term_mask(values, op, arg):
    """The truth value of one term on every entry of ``values`` (u32)."""
    v = np.asarray(values, dtype=np.uint32).astype(np.uint64)      # (u64: no comparison or mask wraps)
    if op in ("in", "not in"):
        hit = np.isin(v, np.array(sorted({int(x) for x in arg}), dtype=np.uint64))
        return ~hit if op == "not in" else hit
    if op in ("range", "not range"):
        lo, hi = int(arg[0]), int(arg[1])
        hit = (v >= np.uint64(lo)) & (v <= np.uint64(hi))
        return ~hit if op == "not range" else hit
    mask = np.uint64(int(arg))
    if op in ("any_bits", "no_bits"):
        hit = (v & mask) != 0
        return ~hit if op == "no_bits" else hit
    if op in ("all_bits", "not all_bits"):
        hit = (v & mask) == mask
        return ~hit if op == "not all_bits" else hit
    raise ValueError(f"unknown op {op!r}")


def where_mask(columns, where, n):
    """The rows of [0, n) on which every term holds.  ``columns``: {column: u32 values (n,)}; a column that is absent
    reads 0 everywhere.  No term: every row."""
    mask = np.ones(n, dtype=bool)
    zeros = np.zeros(n, dtype=np.uint32)
    for column, op, arg in where:
        mask &= term_mask(columns.get(column, zeros), op, arg)
    return mask

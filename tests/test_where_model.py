"""CPU: the numpy model of the ``where`` predicate (tests/where_model.py) against hand-written truth tables, for every
op and its negation, with the edge values 0, 0x80000000 and 0xFFFFFFFF, a > b ranges, mask 0 and the empty set."""
import numpy as np
import pytest

from where_model import OPS, term_mask, where_mask

T, F = True, False
HI, TOP = 0x80000000, 0xFFFFFFFF
V = np.array([0, 1, 2, 7, HI, TOP], dtype=np.uint32)

# (op, arg, the op's truth value on V); the negated op must give the complement
CASES = [
    ("in", [1, 7], [F, T, F, T, F, F]),
    ("in", [7, 1, 7, 7], [F, T, F, T, F, F]),            # order and repeats do not matter
    ("in", [0], [T, F, F, F, F, F]),
    ("in", [HI, TOP], [F, F, F, F, T, T]),
    ("in", [], [F, F, F, F, F, F]),                      # the empty set is never true
    ("in", [3, 4, 5], [F, F, F, F, F, F]),
    ("in", [0, 1, 2, 7, HI, TOP], [T, T, T, T, T, T]),
    ("range", (1, 7), [F, T, T, T, F, F]),
    ("range", (0, 0), [T, F, F, F, F, F]),
    ("range", (0, TOP), [T, T, T, T, T, T]),
    ("range", (HI, TOP), [F, F, F, F, T, T]),
    ("range", (TOP, TOP), [F, F, F, F, F, T]),
    ("range", (2, HI), [F, F, T, T, T, F]),
    ("range", (7, 1), [F, F, F, F, F, F]),               # a > b: never true
    ("range", (TOP, 0), [F, F, F, F, F, F]),
    ("any_bits", 1, [F, T, F, T, F, T]),
    ("any_bits", 6, [F, F, T, T, F, T]),
    ("any_bits", HI, [F, F, F, F, T, T]),
    ("any_bits", TOP, [F, T, T, T, T, T]),
    ("any_bits", 0, [F, F, F, F, F, F]),                 # mask 0: no bit can be set
    ("all_bits", 3, [F, F, F, T, F, T]),
    ("all_bits", 7, [F, F, F, T, F, T]),
    ("all_bits", HI | 1, [F, F, F, F, F, T]),
    ("all_bits", TOP, [F, F, F, F, F, T]),
    ("all_bits", 0, [T, T, T, T, T, T]),                 # mask 0: nothing is asked
]
NEGATED = {"in": "not in", "range": "not range", "any_bits": "no_bits", "all_bits": "not all_bits"}


@pytest.mark.parametrize("op,arg,want", CASES)
def test_every_op_and_its_negation(op, arg, want):
    want = np.array(want)
    assert term_mask(V, op, arg).tolist() == want.tolist()
    assert term_mask(V, NEGATED[op], arg).tolist() == (~want).tolist()


def test_the_cases_cover_every_op():
    assert {op for op, _, _ in CASES} | {NEGATED[op] for op, _, _ in CASES} == set(OPS)
    with pytest.raises(ValueError):
        term_mask(V, "like", 1)


def test_terms_are_anded_and_absent_columns_read_zero():
    cols = {0: V, 2: V[::-1].copy()}
    n = len(V)
    assert where_mask(cols, [], n).all()
    # two terms on one column: 1 <= v <= HI and bit 0 set -> 1, 7
    assert where_mask(cols, [(0, "range", (1, HI)), (0, "any_bits", 1)], n).tolist() == [F, T, F, T, F, F]
    # two columns: v0 in {0, 1, 2} and v2 (= V reversed: TOP, HI, 7, 2, 1, 0) >= HI -> rows 0, 1
    assert where_mask(cols, [(0, "in", [0, 1, 2]), (2, "range", (HI, TOP))], n).tolist() == [T, T, F, F, F, F]
    # column 1 is absent: 0 everywhere
    assert where_mask(cols, [(1, "in", [0])], n).all() and not where_mask(cols, [(1, "not in", [0])], n).any()
    assert where_mask(cols, [(1, "all_bits", 0), (1, "no_bits", TOP), (1, "range", (0, 0))], n).all()
    assert not where_mask(cols, [(0, "in", [1]), (1, "any_bits", TOP)], n).any()
    # the order of the terms does not matter
    w = [(0, "not in", [7]), (2, "not range", (0, 1)), (0, "no_bits", HI)]
    assert where_mask(cols, w, n).tolist() == where_mask(cols, w[::-1], n).tolist() == [T, T, T, F, F, F]

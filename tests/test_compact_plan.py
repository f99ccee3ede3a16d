"""CPU: the host planner of the in-place compaction (svs_amd/csrc/compact.h, through svs_internal_compact_plan).

svs_index_compact moves live rows down over tombstoned ones inside one HBM buffer.  Within a launch a destination
may be another row's source and workgroups run in any order, so correctness rests on the plan: ascending contiguous
steps, DIRECT only where the destination range ends before the source range begins, BOUNCE through a buffer of
bounce_rows rows otherwise.  Each plan is simulated on arange(n) one element at a time, in forward AND reverse order
inside a step, reading at the moment of the write: a legal plan gives arange(n)[live] either way."""
import itertools

import numpy as np
import pytest

from svs_amd import _native

DIRECT, BOUNCE = 0, 1


def plan(dead, n, bounce_rows):
    lib = _native.load()
    dead = np.ascontiguousarray(dead, dtype=np.uint32)
    total = int(lib.svs_internal_compact_plan(dead.ctypes.data, len(dead), n, bounce_rows, None, 0))
    assert total >= 0, _native.last_error()
    steps = np.zeros((max(total, 1), 3), dtype=np.int64)
    assert int(lib.svs_internal_compact_plan(dead.ctypes.data, len(dead), n, bounce_rows, steps.ctypes.data, total)) == total
    return steps[:total]


def sources(dead, n):
    """src[p] for every destination p < n_live."""
    live = np.ones(n, dtype=bool)
    live[dead] = False
    return np.flatnonzero(live)


def check_plan(steps, dead, n, bounce_rows):
    src = sources(dead, n)
    n_live = len(src)
    if len(dead) == 0 or dead[0] >= n_live:
        assert len(steps) == 0
        return src
    pos = int(dead[0])
    for kind, dst0, count in steps.tolist():
        assert dst0 == pos and count >= 1, (steps, dead)
        assert kind in (DIRECT, BOUNCE)
        if kind == DIRECT:
            assert dst0 + count <= src[dst0], (kind, dst0, count, dead)
        else:
            assert count <= bounce_rows
        pos = dst0 + count
    assert pos == n_live, (steps, dead, n)
    return src


def simulate(steps, src, n, reverse):
    a = np.arange(n)
    for kind, dst0, count in steps.tolist():
        order = range(dst0 + count - 1, dst0 - 1, -1) if reverse else range(dst0, dst0 + count)
        if kind == DIRECT:
            for p in order:
                a[p] = a[src[p]]
        else:
            buf = np.empty(count, dtype=a.dtype)
            for p in order:
                buf[p - dst0] = a[src[p]]
            for p in order:
                a[p] = buf[p - dst0]
    return a[:len(src)]


def simulate_vectorised(steps, src, n):
    """The same for long arrays.  A DIRECT step was checked to have disjoint source and destination ranges, so one
    fancy-indexed assignment is what any element order gives."""
    a = np.arange(n)
    for kind, dst0, count in steps.tolist():
        a[dst0:dst0 + count] = a[src[dst0:dst0 + count]].copy()
    return a[:len(src)]


@pytest.mark.parametrize("n", range(0, 13))
def test_every_pattern_of_small_indexes(n):
    for bits in itertools.product((False, True), repeat=n):
        dead = np.flatnonzero(np.array(bits, dtype=bool)).astype(np.uint32)
        for bounce_rows in (1, 2, 3):
            steps = plan(dead, n, bounce_rows)
            src = check_plan(steps, dead, n, bounce_rows)
            for reverse in (False, True):
                got = simulate(steps, src, n, reverse)
                assert np.array_equal(got, src), (n, dead, bounce_rows, reverse, steps)


N_BIG, BOUNCE_BIG = 100_000, 64
BIG = {
    "quarter": lambda rng: np.sort(rng.choice(N_BIG, N_BIG // 4, replace=False)),
    "row0": lambda rng: np.array([0]),
    "run_at_start": lambda rng: np.arange(50_000),
    "last_row": lambda rng: np.array([N_BIG - 1]),
    "all": lambda rng: np.arange(N_BIG),
    "none": lambda rng: np.array([], dtype=np.int64),
}


@pytest.mark.parametrize("name", sorted(BIG))
def test_large_patterns(name):
    dead = BIG[name](np.random.default_rng(7)).astype(np.uint32)
    steps = plan(dead, N_BIG, BOUNCE_BIG)
    src = check_plan(steps, dead, N_BIG, BOUNCE_BIG)
    assert len(steps) < 2 * -(-N_BIG // BOUNCE_BIG) + 64, len(steps)
    assert np.array_equal(simulate_vectorised(steps, src, N_BIG), src)
    kinds = set(steps[:, 0].tolist())
    if name == "row0":
        assert kinds == {BOUNCE}                       # the gap never grows past one row
    if name == "run_at_start":
        assert kinds == {DIRECT} and len(steps) == 1   # 50,000 rows of room from the start
    if name == "quarter":
        assert kinds == {DIRECT, BOUNCE}


def test_bad_lists_are_refused():
    lib = _native.load()
    for dead, n, b in (([3, 3], 8, 2), ([5, 2], 8, 2), ([8], 8, 2), ([1], 8, 0)):
        d = np.array(dead, dtype=np.uint32)
        assert lib.svs_internal_compact_plan(d.ctypes.data, len(d), n, b, None, 0) == _native.SVS_ERR_INVALID


def test_plan_written_up_to_cap_only():
    lib = _native.load()
    dead = np.array([0], dtype=np.uint32)
    steps = np.full((4, 3), -7, dtype=np.int64)
    assert lib.svs_internal_compact_plan(dead.ctypes.data, 1, 10, 2, steps.ctypes.data, 2) == 5
    assert steps[:2].tolist() == [[BOUNCE, 0, 2], [BOUNCE, 2, 2]] and (steps[2:] == -7).all()

"""CPU: the numpy model of the per-label breakdown (by_label_model.py) on hand-written cases."""
import numpy as np

import by_label_model
from by_label_model import by_label


def _lists(res):
    l, s, r, t, g = res
    return l.tolist(), s.tolist(), r.tolist(), t.tolist(), g


#         row:   0    1    2    3    4    5    6    7
S = np.array([0.5, 0.9, 0.1, 0.9, -0.2, 0.3, 0.9, 0.0], dtype=np.float32)
L = np.array([7,   3,   7,   3,   9,    0,   5,   9], dtype=np.uint32)


def test_groups_counts_and_order():
    # label 5: row 6 (0.9); label 3: rows 1, 3 (0.9 twice: row 3 wins); label 7: rows 0, 2; label 9: rows 4, 7; label 0: row 5
    # equal best scores are ordered by row descending: 5 (row 6) before 3 (row 3)
    assert _lists(by_label(S, L, None, [3, 5, 7, 9, 0], None, 10)) == (
        [5, 3, 7, 0, 9], [S[6], S[3], S[0], S[5], S[7]], [6, 3, 0, 5, 7], [1, 2, 2, 1, 2], 5)
    # k cuts the list, not the group count; k <= 0 only counts
    assert _lists(by_label(S, L, None, [3, 5, 7, 9, 0], None, 2)) == ([5, 3], [S[6], S[3]], [6, 3], [1, 2], 5)
    for k in (0, -3):
        assert _lists(by_label(S, L, None, [3, 5, 7, 9, 0], None, k)) == ([], [], [], [], 5)
    # order and repeats of the set do not matter; labels nobody has, and stored labels outside the set, are absent
    a = by_label(S, L, None, [9, 3, 3, 4, 9, 100], None, 10)
    assert _lists(a) == _lists(by_label(S, L, None, [3, 4, 9, 100], None, 10)) == ([3, 9], [S[3], S[7]], [3, 7], [2, 2], 2)
    assert _lists(by_label(S, L, None, [], None, 10)) == ([], [], [], [], 0)
    assert a[0].dtype == np.uint32 and a[1].dtype == np.float32 and a[2].dtype == np.int64 and a[3].dtype == np.int64


def test_cut_offs_are_made_in_key_space():
    # inclusive at a row's own score; the next float above it drops the row
    assert _lists(by_label(S, L, None, [7], np.float32(0.5), 5)) == ([7], [S[0]], [0], [1], 1)
    assert by_label(S, L, None, [7], np.nextafter(np.float32(0.5), np.float32(1)), 5)[4] == 0
    # -0.0 and +0.0 are one cut-off (row 7 scores +0.0)
    for cut in (np.float32(0.0), np.float32(-0.0)):
        assert _lists(by_label(S, L, None, [9, 7], cut, 5)) == ([7, 9], [S[0], S[7]], [0, 7], [2, 1], 2)
    s = S.copy()
    s[7] = np.float32(-0.0)
    assert _lists(by_label(s, L, None, [9], np.float32(0.0), 5))[2:] == ([7], [1], 1)
    # -inf and None admit every live row; +inf admits none
    assert _lists(by_label(S, L, None, [9], -np.inf, 5)) == _lists(by_label(S, L, None, [9], None, 5)) == ([9], [S[7]], [7], [2], 1)
    assert by_label(S, L, None, [3, 5, 7, 9, 0], np.inf, 5)[4] == 0
    # a NaN score qualifies for every cut-off and sorts first
    s = S.copy()
    s[4] = np.nan
    l, sc, r, t, g = by_label(s, L, None, [3, 9], np.inf, 5)
    assert (l.tolist(), r.tolist(), t.tolist(), g) == ([9], [4], [1], 1) and np.isnan(sc[0])
    assert by_label(s, L, None, [3, 9], np.float32(0.8), 5)[0].tolist() == [9, 3]


def test_dead_rows_and_missing_column():
    dead = np.zeros(8, dtype=bool)
    dead[3] = True                                           # the best row of label 3: the runner-up takes over
    assert _lists(by_label(S, L, dead, [3, 5], None, 5)) == ([5, 3], [S[6], S[1]], [6, 1], [1, 1], 2)
    dead[1] = True                                           # every row of label 3: the label leaves G
    assert _lists(by_label(S, L, dead, [3, 5], None, 5)) == ([5], [S[6]], [6], [1], 1)
    # no column: label 0 holds every live row
    assert _lists(by_label(S, None, dead, [0], None, 5)) == ([0], [S[6]], [6], [6], 1)
    assert by_label(S, None, None, [1, 2], None, 5)[4] == 0
    # a dead row never enters through its score: -inf cut-off
    assert by_label(S, L, dead, [3], -np.inf, 5)[4] == 0


def test_score_key_is_above_models():
    import above_model
    assert by_label_model.score_key is above_model.score_key

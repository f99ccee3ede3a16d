"""Host half of the top-k stage's route tests: the case table (select_cases.py) against the route model (select_model.py).
No GPU.  A case whose input no longer takes the route it names -- after a constant of select.h moved, or a seed changed --
fails here, and so does a route that lost its last case: tests/test_select_routes_gpu.py pins a route only through the
cases this file holds to it."""
import numpy as np
import pytest

import select_cases as sc
import select_model as sm


@pytest.mark.parametrize("case", sc.SCORE_CASES, ids=lambda c: c.name)
def test_score_case_takes_its_route(case):
    v = case.gen()
    assert v.dtype == np.float32 and v.ndim == 1
    r = sm.route_scores(v, case.k)
    assert r.name == case.route, (case.why, r)
    if case.emit is not None:
        assert r.emit == case.emit, (case.why, r)
    assert np.array_equal(case.gen().view(np.uint32), v.view(np.uint32)), "the generator must be seeded"


@pytest.mark.parametrize("case", sc.CAND_CASES, ids=lambda c: c.name)
def test_candidate_case_takes_its_route(case):
    keys, claim = case.gen()
    assert keys.dtype == np.uint64 and keys.size == min(claim, sm.CAND_CAP)
    rows = keys & np.uint64(0xFFFFFFFF)
    assert np.unique(rows).size == rows.size, "rows are unique"
    assert keys.size == 0 or int(rows.max()) < sc.CAND_INDEX_ROWS
    assert keys.size == 0 or int((keys >> np.uint64(32)).min()) > 0, "a real key is never 0"
    r = sm.route_candidates(keys, claim, case.count, sc.dead_mask() if case.dead else None)
    assert r.name == case.route, (case.why, r)
    if case.emit is not None:
        assert r.emit == case.emit, (case.why, r)


@pytest.mark.parametrize("case", sc.KTH_CASES, ids=lambda c: c.name)
def test_kth_case_takes_its_route(case):
    v = case.gen()
    r = sm.route_kth(v, case.k, case.misaligned)
    assert r.name == case.route, (case.why, r)


def test_every_route_has_a_case():
    """Set comparisons: every route the model can name is some case's verdict, and no case relies on an undetermined one."""
    assert {c.route for c in sc.SCORE_CASES} == sm.SCORE_ROUTES
    assert {c.route for c in sc.CAND_CASES} == sm.CANDIDATE_ROUTES
    assert {c.route for c in sc.KTH_CASES} == sm.KTH_ROUTES
    assert sm.UNDETERMINED not in sm.SCORE_ROUTES
    # both emit forms, per final-kernel route that has both
    for route in (sm.D, sm.DIRECT, sm.REG_RADIX, sm.CAND_RADIX, sm.RAW_FLAG):
        assert {c.emit for c in sc.SCORE_CASES if c.route == route} >= {sm.RANK, sm.BITONIC}, route
    assert {sm.route_candidates(*c.gen(), c.count, sc.dead_mask() if c.dead else None).emit
            for c in sc.CAND_CASES if c.route == sm.MAXIMA} >= {sm.RANK, sm.BITONIC}
    # the streaming branch by size and by alignment
    assert {c.misaligned for c in sc.KTH_CASES if c.route == sm.STREAM} == {False, True}


def test_mixes_name_cases_of_one_shape():
    by_name = {c.name: c for c in sc.SCORE_CASES}
    for name, members in sc.SCORE_MIXES.items():
        shapes = {by_name[m].gen().size for m in members}
        assert len(shapes) == 1 and len(members) >= 3, name
    # a path A mix holds every path A route
    assert {by_name[m].route for m in sc.SCORE_MIXES["A-n40000-k100"]} == sm.SCORE_ROUTES - {sm.D, sm.B, sm.WINDOW}
    cands = {c.name: c for c in sc.CAND_CASES}
    for name, members in sc.CAND_MIXES.items():
        assert len({(cands[m].count, cands[m].dead) for m in members}) == 1, name
    assert {cands[m].route for ms in sc.CAND_MIXES.values() for m in ms} == sm.CANDIDATE_ROUTES
    kth = {c.name: c for c in sc.KTH_CASES}
    for name, (members, _) in sc.KTH_MIXES.items():
        assert len({(kth[m].gen().size, kth[m].k) for m in members}) == 1 and len(members) == 4, name
    assert {kth[m].route for m in sc.KTH_MIXES["mix-16384-k100"][0]} == sm.KTH_ROUTES - {sm.STREAM}


def test_radix_select_returns_at_the_pass_the_case_names():
    """The tie cases are there for block_radix_select's last pass and for its early exits: hold their reasons to the model."""
    by_name = {c.name: c for c in sc.SCORE_CASES}
    for name, shift in sc.RADIX_EXIT.items():
        c = by_name[name]
        v = c.gen()
        assert sm.route_scores(v, c.k).name in (sm.RAW_FLAG, sm.RAW_OVERFLOW)     # the select runs over the raw scores
        assert sm.radix_exit_shift(sm.make_keys(v, np.arange(v.size)), c.k) == shift, name
    assert {0, 9, 53} <= set(sc.RADIX_EXIT.values()), "the last pass, a middle-pass exit and a first-pass exit"


def test_constants_mirror_select_h():
    """The model's constants are copies: read the originals out of svs_amd/csrc/select.h, so that a limit that moves there
    (as SEL_KMAX once did, 1024 -> 2048, unnoticed by two tests) fails here."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "svs_amd", "csrc", "select.h")
    with open(path) as f:
        src = f.read()

    def const(name):
        m = re.search(r"constexpr\s+(?:int|uint32_t)\s+" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*;", src)
        assert m, f"{name} is no longer a plain constexpr literal in select.h"
        return int(m.group(1), 0)

    assert sm.SEL_KMAX == const("SEL_KMAX") and sm.SORT_CAP == const("SORT_CAP") and sm.CAND_CAP == const("CAND_CAP")
    assert sm.WBINS == const("WBINS") and sm.WTOP == const("WTOP") and sm.WBASE == const("WTOP") - (const("WBINS") - 1)
    assert re.search(r"WBASE\s*=\s*WTOP\s*-\s*\(WBINS\s*-\s*1\)", src)
    assert sm.FINAL_THREADS == const("FINAL_THREADS") and sm.FINAL_DIRECT == const("FINAL_DIRECT")
    assert sm.FINAL_REG_MAX == const("FINAL_THREADS") * const("FINAL_REG_KEYS")
    assert sm.PK_LIST == const("PK_LIST") and sm.PK_REG_MAX == const("FINAL_THREADS") * const("PK_REGS")
    assert const("RS_BINS") == 2048, "radix_exit_shift: 11 bits per pass"
    # SelHeader is four 32-bit words in front of the histogram
    hdr = re.search(r"struct SelHeader \{(.*?)\};", src, re.S).group(1)
    words = sum(len(m.group(1).split(",")) for m in re.finditer(r"uint32_t\s+([^;]+);", hdr))
    assert sm.SCR_WORDS == words + const("WBINS") and re.search(r"SCR_WORDS\s*=\s*sizeof\(SelHeader\)\s*/\s*4\s*\+\s*WBINS", src)


def test_undetermined_is_reported_not_guessed():
    """5000 distinct candidates in one bin, count 100: whether the pivot of the thread maxima overflows the sort depends on
    which thread the filter handed which candidate to."""
    v = sc.one_bin(sc.N_A, 90, m=5000)
    assert sm.route_scores(v, 100).name == sm.UNDETERMINED
    assert sm.route_scores(v, 300).name == sm.REG_RADIX


EDGE_VALUES = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 2.0, np.nextafter(np.float32(2.0), np.float32(0)),
                        2.0 ** -31, np.nextafter(np.float32(2.0 ** -31), np.float32(0)), 2.0 ** -31 * (1 + 1 / 128),
                        1e-40, -1e-40, 1.4e-45, -1.4e-45, 3.4028235e38, -3.4028235e38, 1.1754944e-38, 0.75, 1000.0],
                       dtype=np.float32)


def test_key_round_trip_and_order():
    k = sm.score_key(EDGE_VALUES)
    back = sm.key_score(k)
    want = EDGE_VALUES.copy()
    want[1] = 0.0                                             # -0 comes back as +0
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
    assert k[0] == k[1] == 0x80000000
    assert int(k.min()) >= 0x007FFFFF, "a real key is never 0"
    # the unsigned key order is the float order
    order = np.argsort(EDGE_VALUES, kind="stable")
    assert np.all(np.diff(k[order].astype(np.int64)) >= 0)
    # every NaN, whatever its sign and payload, is the maximum and comes back canonical
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    assert np.all(sm.score_key(nans) == sm.NAN_KEY)
    assert np.all(sm.key_score(sm.score_key(nans)).view(np.uint32) == 0x7FC00000)


def test_window_bins():
    def b(x):
        return int(sm.window_bin(sm.score_key(np.array([x], dtype=np.float32)))[0])
    assert sm.WBASE == sm.WTOP - (sm.WBINS - 1) == 0xB001
    assert b(2.0) == sm.WBINS - 1 and b(1000.0) == sm.WBINS - 1 and b(np.inf) == sm.WBINS - 1 and b(np.nan) == sm.WBINS - 1
    assert b(np.nextafter(np.float32(2.0), np.float32(0))) == sm.WBINS - 2
    assert b(2.0 ** -31 * (1 + 1 / 128)) == 0, "the lowest bin starts one 128th of an octave above 2^-31"
    assert b(2.0 ** -31) == -1 and b(1e-40) == -1 and b(0.0) == -1 and b(-1.0) == -1
    assert b(0.75) == b(0.7525) and b(0.75) != b(0.754), "128 bins per octave"


def test_expected_scores_is_the_oracle_order():
    """expected_scores: oracle.total_order_top_k's rows (score descending, NaN first, ties by row descending); scores as
    the kernels emit them."""
    v = np.array([0.5, np.nan, -0.0, 0.0, 0.5, -np.inf, np.nan], dtype=np.float32)
    bits, rows = sm.expected_scores(v, 9, row_offset=10)
    assert rows.tolist() == [16, 11, 14, 10, 13, 12, 15, -1, -1]
    f = bits.view(np.float32)
    assert np.isnan(f[:2]).all() and bits[0] == 0x7FC00000 and f[2] == f[3] == 0.5
    assert bits[4] == bits[5] == 0 and f[6] == -np.inf and np.isneginf(f[7:]).all()

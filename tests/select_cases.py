"""The case table of the top-k stage's routes, as data: which seeded input must take which route (select_model.py), and
why.  tests/test_select_model.py holds every entry to the model on the CPU and checks that every route the model can name
has a case; tests/test_select_routes_gpu.py runs the entries bit-exact on the device.

Path A shapes: n = 12,289 = 8192 + 4097 is two histogram workgroups, the second partly empty, n % 4 == 1; only the
candidate-list overflow needs more than CAND_CAP rows (40,000).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import select_model as sm

N_A = 12289
N_BIG = 40000
F32 = np.float32

# hook: "scores" | "cand" | "kth"; gen() -> the input (see each table); emit: RANK / BITONIC / None (not asserted)
Case = namedtuple("Case", "name gen k route emit why")


def _rng(seed):
    return np.random.default_rng(seed)


# ---- score vectors ----------------------------------------------------------------------------------------
def gauss(n, seed, scale=0.3):
    return (_rng(seed).standard_normal(n) * scale).astype(F32)


def one_bin(n, seed, m=3000, top=40):
    """m distinct values inside the window bin [0.75, 0.75390625), `top` rows at 1.5, the rest well below"""
    rng = _rng(seed)
    v = (rng.standard_normal(n) * 0.1).astype(F32)
    at = rng.permutation(n)[: m + top]
    v[at[:m]] = np.linspace(0.75, 0.7525, m, endpoint=False).astype(F32)
    v[at[m:]] = 1.5
    return v


def ties(n, seed, m=6000, top=40, val=0.9):
    rng = _rng(seed)
    v = (rng.standard_normal(n) * 0.1).astype(F32)
    at = rng.permutation(n)[: m + top]
    v[at[:m]] = val
    v[at[m:]] = 1.5
    return v


def negative(n, seed):
    return (-np.abs(_rng(seed).standard_normal(n)) - 1e-3).astype(F32)


def few_positive(n, seed, m=99):
    rng = _rng(seed)
    v = negative(n, seed + 1)
    v[rng.permutation(n)[:m]] = (rng.random(m) * 0.9 + 0.05).astype(F32)
    return v


def equal(n, val=0.25):
    return np.full(n, val, dtype=F32)


def best_last(n, seed):
    v = gauss(n, seed)
    v[-1] = 1.75
    return v


def value_edges(n, seed):
    """NaN in the first, a middle and the last row, +-inf, +-0 and denormals among Gaussian scores"""
    v = gauss(n, seed)
    v[0] = v[n // 2] = v[-1] = np.nan
    v[1], v[n - 2] = np.inf, np.inf
    v[2], v[n - 3] = -np.inf, -np.inf
    if n > 16:
        v[3:7] = [0.0, -0.0, 0.0, -0.0]
        v[7:9] = [1e-40, -1e-40]
    return v


def edges_nonpositive(n, seed):
    v = value_edges(n, seed)
    pos = np.isfinite(v) & (v > 0)
    v[pos] = -v[pos]
    return v


def zero_ties(n, seed):
    """the best scores are 50 zeros of both signs (outside the window) above negatives: the tie falls to the row"""
    rng = _rng(seed)
    v = negative(n, seed + 1)
    at = rng.permutation(n)[:50]
    v[at[:25]] = 0.0
    v[at[25:]] = -0.0
    return v


def above_two(n, seed, m):
    """m scores in [2, 1000] and +inf: all clamp into the top bin"""
    rng = _rng(seed)
    v = gauss(n, seed + 1)
    at = rng.permutation(n)[:m]
    v[at] = (2.0 + rng.random(m) * 998.0).astype(F32)
    v[at[0]] = np.inf
    return v


def below_window(n, seed, inside=50, below=150):
    """`inside` scores inside the window, `below` positive ones just under 2^-31 (outside it), the rest negative"""
    rng = _rng(seed)
    v = negative(n, seed + 1)
    at = rng.permutation(n)[: inside + below]
    v[at[:inside]] = (rng.random(inside) * 0.5 + 0.1).astype(F32)
    v[at[inside:]] = (2.0 ** -31 * (0.25 + 0.75 * rng.random(below))).astype(F32)
    return v


def denormals(n, seed, m=200):
    rng = _rng(seed)
    v = negative(n, seed + 1)
    at = rng.permutation(n)[:m]
    v[at] = (rng.integers(1, 1 << 22, m).astype(np.uint32)).view(F32)    # positive denormals, distinct-ish bit patterns
    return v


def tie_block(n, seed, row0, m):
    """m tied best scores at rows row0 .. row0 + m - 1 above negatives (block_radix_select over the raw scores)"""
    v = negative(n, seed)
    v[row0: row0 + m] = -5e-4
    return v


def tie_spread(n, seed, step):
    """tied best scores every `step` rows above negatives: each winner alone in its bucket of the row bits"""
    v = negative(n, seed)
    v[::step] = -5e-4
    return v


def d_vector(n, seed=40):
    """path D input: the value edges where they fit, else a few Gaussian scores"""
    if n >= 16:
        return value_edges(n, seed + n)
    v = gauss(n, seed + n)
    if n == 3:
        v[:] = [0.0, np.nan, -0.0]
    return v


SCORE_CASES = [
    # --- the route table
    Case("gauss-k1", lambda: gauss(N_A, 1), 1, sm.DIRECT, sm.RANK, "n_cand is the top bin's handful"),
    Case("gauss-k100", lambda: gauss(N_A, 1), 100, sm.DIRECT, sm.RANK, "k + the few keys sharing bin b*: <= 256 slots"),
    Case("gauss-k255", lambda: gauss(N_A, 1), 255, sm.DIRECT, None, "count just under the 256 | 257 boundary"),
    Case("gauss-k256", lambda: gauss(N_A, 1), 256, sm.DIRECT, sm.BITONIC, "count 256: the list spills over 256 slots"),
    Case("gauss-k257", lambda: gauss(N_A, 1), 257, sm.DIRECT, sm.BITONIC, "count 257"),
    Case("gauss-k1023", lambda: gauss(N_A, 1), 1023, sm.DIRECT, sm.BITONIC, "n_cand 1023: the longest lists sorted as they are"),
    Case("gauss-k2047", lambda: gauss(N_A, 1), 2047, sm.WINDOW, sm.BITONIC, "count - 1 of the path A | B boundary"),
    Case("gauss-k2048", lambda: gauss(N_A, 1), 2048, sm.WINDOW, sm.BITONIC, "n_cand > 1024, count > 256: window pass"),
    Case("gauss-k2049", lambda: gauss(N_A, 1), 2049, sm.B, None, "count > SEL_KMAX"),
    Case("onebin-k10", lambda: one_bin(N_A, 2), 10, sm.DIRECT, sm.RANK, "the 40 rows at 1.5 hold the 10th best"),
    Case("onebin-k41", lambda: one_bin(N_A, 2), 41, sm.MAXIMA, None, "3040 candidates, count <= 256"),
    Case("onebin-k100", lambda: one_bin(N_A, 2), 100, sm.MAXIMA, None, "3040 candidates, count <= 256"),
    Case("onebin-k256", lambda: one_bin(N_A, 2), 256, sm.MAXIMA, None, "count == 256 still takes the pivot"),
    Case("onebin-k257", lambda: one_bin(N_A, 2), 257, sm.WINDOW, sm.BITONIC, "count 257: no pivot"),
    Case("onebin-k1024", lambda: one_bin(N_A, 2), 1024, sm.WINDOW, sm.BITONIC, "3040 candidates fit the sort"),
    Case("ties6000-k41", lambda: ties(N_A, 3), 41, sm.REG_RADIX, sm.RANK, "6000 ties at the 41st place overflow pivot and window"),
    Case("ties6000-k256", lambda: ties(N_A, 3), 256, sm.REG_RADIX, sm.RANK, "count 256 | 257 inside the register radix select"),
    Case("ties6000-k257", lambda: ties(N_A, 3), 257, sm.REG_RADIX, sm.BITONIC, "count > 256: window overflow only"),
    Case("ties6000-k1024", lambda: ties(N_A, 3), 1024, sm.REG_RADIX, sm.BITONIC, "count > 256"),
    Case("onebin9000-k41", lambda: one_bin(N_A, 4, m=9000), 41, sm.CAND_RADIX, sm.RANK, "9040 candidates, distinct: early exit"),
    Case("onebin9000-k1024", lambda: one_bin(N_A, 4, m=9000), 1024, sm.CAND_RADIX, sm.BITONIC, "9040 candidates"),
    Case("ties12000-k100", lambda: ties(N_A, 5, m=12000), 100, sm.CAND_RADIX, sm.RANK, "ties: the radix select's last pass"),
    Case("negative-k100", lambda: negative(N_A, 6), 100, sm.RAW_FLAG, sm.RANK, "nothing inside the window"),
    Case("negative-k2048", lambda: negative(N_A, 6), 2048, sm.RAW_FLAG, sm.BITONIC, "the largest count of the raw fallback"),
    Case("pos99-k100", lambda: few_positive(N_A, 7), 100, sm.RAW_FLAG, sm.RANK, "the window holds 99 < count"),
    Case("pos99-k99", lambda: few_positive(N_A, 7), 99, sm.DIRECT, sm.RANK, "the window holds exactly count"),
    Case("equal40000-k5", lambda: equal(N_BIG), 5, sm.RAW_OVERFLOW, sm.RANK, "40,000 survivors > CAND_CAP; the winners 39,995 .. 39,999 share row >> 9: every radix pass, the last included"),
    # --- sizes: one and two histogram workgroups, full and partly empty, every n % 4
    Case("n4097-k100", lambda: gauss(4097, 8), 100, sm.DIRECT, None, "smallest path A size"),
    Case("n8191-k100", lambda: gauss(8191, 9), 100, sm.DIRECT, None, "one workgroup, one score short"),
    Case("n8192-k100", lambda: gauss(8192, 10), 100, sm.DIRECT, None, "exactly one workgroup"),
    Case("n8193-k100", lambda: gauss(8193, 11), 100, sm.DIRECT, None, "second workgroup holds one score"),
    Case("last-n4097-k1", lambda: best_last(4097, 12), 1, sm.DIRECT, sm.RANK, "n % 4 == 1, best in the last row"),
    Case("last-n4098-k1", lambda: best_last(4098, 13), 1, sm.DIRECT, sm.RANK, "n % 4 == 2, best in the last row"),
    Case("last-n4099-k3", lambda: best_last(4099, 14), 3, sm.DIRECT, sm.RANK, "n % 4 == 3, best in the last row"),
    # --- values
    Case("edges-k100", lambda: value_edges(N_A, 15), 100, sm.DIRECT, None, "NaN first / middle / last, +-inf, +-0, denormals"),
    Case("edges-nonpositive-k100", lambda: edges_nonpositive(N_A, 15), 100, sm.RAW_FLAG, sm.RANK,
         "3 NaN + 2 inf inside the window, then zeros of both signs, a negative denormal, negatives"),
    Case("zeroties-k30", lambda: zero_ties(N_A, 16), 30, sm.RAW_FLAG, sm.RANK, "+0 / -0 tie, by row"),
    Case("above2-300-k100", lambda: above_two(N_A, 17, 300), 100, sm.DIRECT, sm.BITONIC, "top-bin clamp: 300 scores >= 2 share one bin"),
    Case("above2-1500-k100", lambda: above_two(N_A, 18, 1500), 100, sm.MAXIMA, None, "top-bin clamp, register route"),
    Case("above2-1500-k300", lambda: above_two(N_A, 18, 1500), 300, sm.WINDOW, sm.BITONIC, "every survivor in the top bin"),
    Case("below-window-k100", lambda: below_window(N_A, 19), 100, sm.RAW_FLAG, sm.RANK, "positives under 2^-31 are outside the window"),
    Case("below-window-k50", lambda: below_window(N_A, 19), 50, sm.DIRECT, sm.RANK, "the window holds exactly count"),
    Case("denormals-k100", lambda: denormals(N_A, 20), 100, sm.RAW_FLAG, sm.RANK, "denormal winners keep their bits"),
    Case("tieblock-low9-k100", lambda: tie_block(N_A, 21, 1024, 300), 100, sm.RAW_FLAG, sm.RANK,
         "300 ties in rows 1024..1323 differ only in the low 9 row bits: block_radix_select's last pass"),
    Case("tieblock-whole-k512", lambda: tie_block(N_A, 22, 2048, 512), 512, sm.RAW_FLAG, sm.BITONIC,
         "the ties' exponent is theirs alone: the first pass (shift 53) takes their whole bucket and returns"),
    Case("tieblock-bucket-k512", lambda: tie_block(N_A, 36, 2048, 1024), 512, sm.RAW_FLAG, sm.BITONIC,
         "1024 ties in rows 2048..3071: the 512 winners, rows 2560..3071, are one whole bucket of the shift-9 pass: it "
         "returns there, without the last pass"),
    Case("tiespread-k5", lambda: tie_spread(N_A, 37, 1000), 5, sm.RAW_FLAG, sm.RANK,
         "13 ties 1000 rows apart: the 5th winner is alone in its shift-9 bucket: early exit in a middle pass"),
    # --- path B: npad = n and npad = 2n - 1, one and several global stages
    Case("B-n4097-k2049", lambda: value_edges(4097, 23), 2049, sm.B, None, "npad = 8192 = 2n - 2: one global stage"),
    Case("B-n8192-k8192", lambda: ties(8192, 24, m=3000), 8192, sm.B, None, "npad = n, whole ranking, ties"),
    Case("B-n8193-k3000", lambda: value_edges(8193, 25), 3000, sm.B, None, "npad = 16,384 = 2n - 2"),
    Case("B-n40000-k2049", lambda: ties(N_BIG, 26, m=6000), 2049, sm.B, None, "npad = 65,536: four merge sizes"),
    Case("B-n8192-edges-k8192", lambda: value_edges(8192, 34), 8192, sm.B, None, "npad = n with NaN, inf and zeros: multi-query mix"),
    Case("B-n8193-negative-k3000", lambda: negative(8193, 35), 3000, sm.B, None, "multi-query mix"),
    Case("B-n4097-k4100", lambda: gauss(4097, 27), 4100, sm.B, None, "k > n on a path A size is path B"),
    # --- the n = 40,000 forms that share one call with the overflow case
    Case("big-gauss-k100", lambda: gauss(N_BIG, 28), 100, sm.DIRECT, None, "multi-query mix"),
    Case("big-onebin-k100", lambda: one_bin(N_BIG, 29), 100, sm.MAXIMA, None, "multi-query mix"),
    Case("big-ties6000-k100", lambda: ties(N_BIG, 33), 100, sm.REG_RADIX, sm.RANK, "multi-query mix"),
    Case("big-onebin9000-k100", lambda: one_bin(N_BIG, 30, m=9000), 100, sm.CAND_RADIX, sm.RANK, "multi-query mix"),
    Case("big-negative-k100", lambda: negative(N_BIG, 31), 100, sm.RAW_FLAG, sm.RANK, "multi-query mix"),
    Case("big-equal-k100", lambda: equal(N_BIG), 100, sm.RAW_OVERFLOW, sm.RANK, "multi-query mix"),
]
# path D: one workgroup reads the scores; 2 .. 4096 sort slots, both emit forms, padding keys (k = n; the device test adds
# k = 1 and k = n + 3)
D_SIZES = (1, 2, 3, 255, 256, 257, 4095, 4096)
SCORE_CASES += [Case(f"D-n{n}", (lambda n=n: d_vector(n)), n, sm.D, sm.RANK if n <= 256 else sm.BITONIC,
                     "path D, value edges") for n in D_SIZES]
# several queries in ONE call (same n and k), each of another route: the blockIdx.y strides and the per-query scratch stride
SCORE_MIXES = {
    "A-n40000-k100": ["big-gauss-k100", "big-onebin-k100", "big-ties6000-k100", "big-onebin9000-k100", "big-negative-k100",
                      "big-equal-k100"],
    "A-n12289-k100": ["gauss-k100", "onebin-k100", "ties12000-k100", "negative-k100", "pos99-k100", "edges-k100"],
    "B-n40000-k2049": ["B-n40000-k2049", "big-gauss-k100", "big-equal-k100"],
    "B-n4097-k2049": ["B-n4097-k2049", "n4097-k100", "last-n4097-k1"],
    "B-n8192-k8192": ["B-n8192-k8192", "B-n8192-edges-k8192", "n8192-k100"],      # npad = n: no padding keys, count = n
    "B-n8193-k3000": ["B-n8193-k3000", "B-n8193-negative-k3000", "n8193-k100"],   # npad = 16,384: three global stages
}
# the pass at which block_radix_select over the raw keys returns (select_model.radix_exit_shift; 0: the last pass, over
# the low 9 row bits): what the reasons of these cases claim
RADIX_EXIT = {"tieblock-low9-k100": 0, "equal40000-k5": 0, "tieblock-whole-k512": 53, "tieblock-bucket-k512": 9, "tiespread-k5": 9}


# ---- candidate lists (mode 3) -------------------------------------------------------------------------------
# gen() -> (keys u64 in upload order, claimed n_cand); rows are < CAND_INDEX_ROWS; DEAD_ROWS are masked in the index the
# tombstone cases run on (their k is the count; `dead` says whether the bitmap is passed)
CAND_INDEX_ROWS = 65536
DEAD_LO, DEAD_HI = 40000, 50000       # masked rows of that index: [DEAD_LO, DEAD_HI)
CandCase = namedtuple("CandCase", "name gen count dead route emit why")


def dead_mask():
    d = np.zeros(CAND_INDEX_ROWS, dtype=bool)
    d[DEAD_LO:DEAD_HI] = True
    return d


def _live_rows(rng, m):
    return rng.permutation(DEAD_LO)[:m]


def cand_gauss(m, seed, claim=None):
    """m positive distinct-ish scores in random order, live rows"""
    rng = _rng(seed)
    s = (np.abs(rng.standard_normal(m)) * 0.3 + 1e-3).astype(F32)
    return sm.make_keys(s, _live_rows(rng, m)), (m if claim is None else claim)


def cand_negative(m, seed):
    rng = _rng(seed)
    return sm.make_keys(negative(m, seed), _live_rows(rng, m)), m


def _thread_major(keys):
    """Upload order in which thread t (which holds keys[t::256]) gets the t-th run of the descending order: the
    per-thread maxima are then every (m / 256)-th key, and the count-th of them lies far down the list."""
    m = keys.size
    per = -(-m // sm.FINAL_THREADS)
    srt = np.sort(keys)[::-1]
    # slot t + 256 j <- the (t * per + j)-th best; the short last rows are filled from what is left
    grid = np.full((per, sm.FINAL_THREADS), -1, dtype=np.int64)
    full = m - (per - 1) * sm.FINAL_THREADS      # threads that hold `per` keys
    pos = 0
    for t in range(sm.FINAL_THREADS):
        mine = per if t < full else per - 1
        grid[:mine, t] = np.arange(pos, pos + mine)
        pos += mine
    flat = grid.reshape(-1)[:m]
    assert (flat >= 0).all() and pos == m
    return srt[flat]


def cand_spread_sorted(m, seed, negative_scores=False):
    """distinct scores spread over many window bins (or all negative), in thread-major descending order"""
    rng = _rng(seed)
    s = (rng.random(m) * 1.89 + 0.01).astype(F32)
    if negative_scores:
        s = -s
    return _thread_major(sm.make_keys(s, _live_rows(rng, m))), m


def cand_ties(m, seed, tied):
    rng = _rng(seed)
    s = (np.abs(rng.standard_normal(m)) * 0.1 + 1e-3).astype(F32)
    s[rng.permutation(m)[:tied]] = 0.9
    return sm.make_keys(s, _live_rows(rng, m)), m


def cand_dead_winners(m, seed, n_dead):
    """the n_dead best candidates are masked rows"""
    rng = _rng(seed)
    s = np.sort((np.abs(rng.standard_normal(m)) * 0.3 + 1e-3).astype(F32))[::-1]
    rows = _live_rows(rng, m)
    rows[:n_dead] = DEAD_LO + rng.permutation(DEAD_HI - DEAD_LO)[:n_dead]
    keys = sm.make_keys(s, rows)
    return keys[rng.permutation(m)], m


def cand_dead_threads(m, seed, live_threads):
    """every candidate of the threads >= live_threads is a masked row: fewer than count thread maxima, pivot 0"""
    rng = _rng(seed)
    s = (np.abs(rng.standard_normal(m)) * 0.3 + 1e-3).astype(F32)
    rows = _live_rows(rng, m)
    gone = (np.arange(m) % sm.FINAL_THREADS) >= live_threads
    rows[gone] = DEAD_LO + rng.permutation(DEAD_HI - DEAD_LO)[: int(gone.sum())]
    return sm.make_keys(s, rows), m


def _sizes():
    out = []
    routes = {0: sm.DIRECT, 1: sm.DIRECT, 255: sm.DIRECT, 256: sm.DIRECT, 257: sm.DIRECT, 1024: sm.DIRECT, 1025: sm.MAXIMA,
              4096: sm.MAXIMA, 4097: sm.MAXIMA, 8192: sm.MAXIMA, 8193: sm.CAND_RADIX, 32768: sm.CAND_RADIX}
    for m, route in routes.items():
        for count in (1, 100, 256):
            r = sm.MARKED if m < count else route
            out.append(CandCase(f"size{m}-c{count}", (lambda m=m: cand_gauss(m, 100 + m)), count, False, r, None,
                                "list size at a route boundary" if m >= count else "fewer keys than count"))
    return out


CAND_CASES = _sizes() + [
    CandCase("claim32769-c100", lambda: cand_gauss(32768, 200, claim=32769), 100, False, sm.MARKED, None, "the list overflowed"),
    CandCase("claim-huge-c1", lambda: cand_gauss(32768, 201, claim=4000000000), 1, False, sm.MARKED, None, "a claim near 2^32"),
    CandCase("sorted8000-c100", lambda: cand_spread_sorted(8000, 202), 100, False, sm.MAXIMA, sm.BITONIC,
             "thread-major order: the pivot keeps ~3100 keys, under the sort's capacity"),
    CandCase("sorted8000-c200", lambda: cand_spread_sorted(8000, 202), 200, False, sm.WINDOW, None,
             "pivot overflow (> 4096 keys at or above it), no crowded bin"),
    CandCase("sorted8000-c256", lambda: cand_spread_sorted(8000, 202), 256, False, sm.WINDOW, None, "pivot overflow, count 256"),
    CandCase("ties5000-c100", lambda: cand_ties(8000, 203, 5000), 100, False, sm.REG_RADIX, sm.RANK,
             "5000 ties overflow the pivot list and the window bin"),
    CandCase("ties5000-c256", lambda: cand_ties(8000, 203, 5000), 256, False, sm.REG_RADIX, sm.RANK, "count 256"),
    CandCase("negsorted8000-c256", lambda: cand_spread_sorted(8000, 204, negative_scores=True), 256, False, sm.REG_RADIX, sm.RANK,
             "all-negative scores: pivot overflow, then an empty window"),
    CandCase("neg2000-c100", lambda: cand_negative(2000, 205), 100, False, sm.MAXIMA, None,
             "negative scores need no window: the pivot works on keys"),
    CandCase("dead-winners-direct-c100", lambda: cand_dead_winners(900, 206, 60), 100, True, sm.DIRECT, None, "60 masked rows lead the list"),
    CandCase("dead-winners-reg-c100", lambda: cand_dead_winners(3000, 207, 300), 100, True, sm.MAXIMA, None, "300 masked rows lead the list"),
    CandCase("dead-winners-radix-c100", lambda: cand_dead_winners(9000, 208, 300), 100, True, sm.CAND_RADIX, sm.RANK, "struck-out keys in the radix select"),
    CandCase("dead-too-many-c100", lambda: cand_dead_winners(150, 209, 100), 100, True, sm.MARKED, None, "50 live keys < count"),
    CandCase("dead-threads-c100", lambda: cand_dead_threads(1100, 210, 50), 100, True, sm.WINDOW, None,
             "50 threads hold live keys: the pivot is 0, the window pass answers"),
    CandCase("dead-unused-c100", lambda: cand_dead_winners(3000, 207, 300), 100, False, sm.MAXIMA, None,
             "the same list without the bitmap: masked rows win"),
]
# several lists in one call (one count): every mode-3 route side by side
CAND_MIXES = {
    "mix-c100": ["size257-c100", "sorted8000-c100", "ties5000-c100", "size8193-c100", "claim32769-c100", "size1-c100", "size4097-c100"],
    "mix-c256": ["sorted8000-c256", "negsorted8000-c256", "size32768-c256", "size255-c256", "ties5000-c256"],
    "mix-dead-c100": ["dead-winners-direct-c100", "dead-too-many-c100", "dead-threads-c100", "dead-winners-radix-c100", "dead-winners-reg-c100"],
}


# ---- k-th value ------------------------------------------------------------------------------------------------
# gen() -> score vector; k; misaligned
KthCase = namedtuple("KthCase", "name gen k misaligned route why")
N_K = 16384


def kth_concentrated(n, seed):
    """150 large values held by 50 threads, 2048 ties at 0.5 in every thread: the 100th thread maximum is the tie value
    (> 1024 keys at or above the pivot), the 100th best is a large value in a sparse bin"""
    rng = _rng(seed)
    v = (rng.standard_normal(n) * 0.05).astype(F32)
    tie_at = np.arange(0, 8192, 4) + 3                              # float4 groups 0..2047: every thread, element 3
    v[tie_at] = 0.5
    big_at = np.array([4 * t + e for t in range(50) for e in range(3)])       # elements 0..2 of the first group of threads 0..49
    v[big_at] = (1.0 + rng.random(big_at.size) * 0.9).astype(F32)
    return v


KTH_CASES = [
    KthCase("gauss-16384-k1", lambda: gauss(N_K, 50), 1, False, sm.MAXIMA, "k = 1"),
    KthCase("gauss-16384-k100", lambda: gauss(N_K, 50), 100, False, sm.MAXIMA, "the usual case"),
    KthCase("gauss-16384-k256", lambda: gauss(N_K, 50), 256, False, sm.WINDOW,
            "k = 256: the pivot is the SMALLEST thread maximum, > 1024 keys at or above it"),
    KthCase("gauss-1024-k256", lambda: gauss(1024, 66), 256, False, sm.MAXIMA, "k = 256 with 4 keys per thread: the pivot list fits"),
    KthCase("gauss-16384-k257", lambda: gauss(N_K, 50), 257, False, sm.WINDOW, "k = 257: no pivot"),
    KthCase("gauss-16384-k2048", lambda: gauss(N_K, 50), 2048, False, sm.WINDOW, "large k"),
    KthCase("gauss-16383-k100", lambda: gauss(16383, 51), 100, False, sm.MAXIMA, "n % 4 == 3: the scalar tail loads"),
    KthCase("edges-16383-k100", lambda: value_edges(16383, 52), 100, False, sm.MAXIMA, "NaN / inf among the best"),
    KthCase("edges-16383-k3", lambda: value_edges(16383, 52), 3, False, sm.MAXIMA, "the k-th best is NaN"),
    KthCase("gauss-1023-k100", lambda: gauss(1023, 53), 100, False, sm.MAXIMA, "every thread holds 3 or 4 keys"),
    KthCase("gauss-257-k100", lambda: gauss(257, 54), 100, False, sm.WINDOW, "65 threads hold keys: pivot 0"),
    KthCase("gauss-257-k1", lambda: gauss(257, 54), 1, False, sm.MAXIMA, "n = 257, k = 1"),
    KthCase("gauss-257-k257", lambda: gauss(257, 54), 257, False, sm.REG_RADIX, "n = k: the minimum, a negative score"),
    KthCase("gauss-100-k100", lambda: gauss(100, 55), 100, False, sm.REG_RADIX, "n = k = 100: 25 threads, negative k-th best"),
    KthCase("gauss-2048-k2048", lambda: gauss(2048, 56), 2048, False, sm.REG_RADIX, "n = k = 2048"),
    KthCase("one-k1", lambda: np.array([-0.0], dtype=F32), 1, False, sm.MAXIMA, "n = k = 1, -0 reads as +0"),
    KthCase("concentrated-k100", lambda: kth_concentrated(N_K, 57), 100, False, sm.WINDOW, "> 1024 keys at or above the pivot, sparse bin"),
    KthCase("ties2000-k100", lambda: ties(N_K, 58, m=2000, top=40), 100, False, sm.REG_RADIX, "> 1024 keys in the k-th's bin"),
    KthCase("negative-k257", lambda: negative(N_K, 59), 257, False, sm.REG_RADIX, "negative k-th best: empty window"),
    KthCase("negative-k100", lambda: negative(N_K, 59), 100, False, sm.MAXIMA, "negative scores need no window: the pivot works on keys"),
    KthCase("zeroties-k30", lambda: zero_ties(N_K, 60), 30, False, sm.MAXIMA, "k-th best is a zero"),
    KthCase("denormals-k257", lambda: denormals(N_K, 61), 257, False, sm.REG_RADIX, "200 denormals above negatives"),
    KthCase("stream-16385-k100", lambda: gauss(16385, 62), 100, False, sm.STREAM, "one row past the register limit"),
    KthCase("stream-16385-k2048", lambda: value_edges(16385, 63), 2048, False, sm.STREAM, "streaming, large k"),
    KthCase("stream-misaligned-5000-k100", lambda: gauss(5000, 64), 100, True, sm.STREAM, "rows one float off a 16-byte boundary"),
    KthCase("stream-misaligned-4999-k257", lambda: value_edges(4999, 65), 257, True, sm.STREAM, "misaligned, n % 4 == 3"),
]
KTH_MIXES = {
    # (the streaming branch is chosen per call -- by n and the alignment -- so it mixes only distributions)
    "mix-16384-k100": (["gauss-16384-k100", "concentrated-k100", "ties2000-k100", "negative-k100"], False),
    "mix-16384-k100-misaligned": (["gauss-16384-k100", "concentrated-k100", "ties2000-k100", "negative-k100"], True),
}

"""Which route of the top-k stage a given input takes: a numpy restatement of the branching rules of
svs_amd/csrc/select.h (and of run_select in svs_amd.hip), written from those rules and not from kernel output.

The stage's ANSWER never depends on the route (every route is exact); the route decides which code produced it.  The case
table (select_cases.py) names a route per case, tests/test_select_model.py holds the table to this model on the CPU, and
tests/test_select_routes_gpu.py runs the cases bit-exact on the device: a route is pinned when a case the model sends
down it passes there.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# ---- constants mirrored from svs_amd/csrc/select.h ----------------------------------------------
SEL_KMAX = 2048        # SEL_KMAX: path A handles count <= SEL_KMAX; above it path B (global bitonic sort)
SORT_CAP = 4096        # SORT_CAP: keys one workgroup sorts in LDS; n <= SORT_CAP is path D
CAND_CAP = 32768       # CAND_CAP: candidate list of one query
FINAL_DIRECT = 1024    # FINAL_DIRECT: lists this short are sorted as they are
FINAL_REG_MAX = 8192   # FINAL_THREADS * FINAL_REG_KEYS: lists read once into registers
FINAL_THREADS = 256    # FINAL_THREADS: also the emit-by-rank limit and the per-thread-maxima limit on count
WBINS = 4096           # WBINS
WTOP = 0xC000          # WTOP: key16 of 2.0f
WBASE = 0xB001         # WBASE = WTOP - (WBINS - 1): key16 just above 2^-31
PK_LIST = 1024         # PK_LIST: keys prefix_kth_kernel lists in LDS
PK_REG_MAX = 16384     # FINAL_THREADS * PK_REGS: prefixes prefix_kth_kernel reads once into registers
SCR_WORDS = 4 + WBINS  # SCR_WORDS: per-query scratch words (SelHeader + histogram)

NAN_KEY = 0xFFFFFFFF

# route names
D, B = "D", "B"
RAW_FLAG, RAW_OVERFLOW = "RAW_FLAG", "RAW_OVERFLOW"
CAND_RADIX, DIRECT = "CAND_RADIX", "DIRECT"
MAXIMA, WINDOW, REG_RADIX = "MAXIMA", "WINDOW", "REG_RADIX"
UNDETERMINED = "REG_UNDETERMINED"
MARKED = "MARKED"
STREAM = "STREAM"
RANK, BITONIC = "RANK", "BITONIC"

SCORE_ROUTES = {D, B, RAW_FLAG, RAW_OVERFLOW, CAND_RADIX, DIRECT, MAXIMA, WINDOW, REG_RADIX}
CANDIDATE_ROUTES = {MARKED, DIRECT, MAXIMA, WINDOW, REG_RADIX, CAND_RADIX}
KTH_ROUTES = {MAXIMA, WINDOW, REG_RADIX, STREAM}

# name: the route; emit: RANK / BITONIC (None where it depends on scheduling, or nothing is emitted by the final kernel);
# flag, n_cand: the header the final kernel reads (None outside path A / mode 3); total: keys that reached the LDS sort
Route = namedtuple("Route", "name emit flag n_cand total")


# ---- keys.h -------------------------------------------------------------------------------------
def score_key(v) -> np.ndarray:
    """f32 -> u32 whose unsigned order is the float order; -0 folds onto +0, any NaN is the maximum."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    u = np.where(u == 0x80000000, 0, u)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(nan, NAN_KEY, k).astype(np.uint32)


def key_score(k) -> np.ndarray:
    """The inverse, as the kernels emit scores: the canonical NaN for the NaN key, +0 for both zeros."""
    k = np.asarray(k, dtype=np.uint32).astype(np.uint64)
    u = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF)
    u = np.where(k == NAN_KEY, 0x7FC00000, u)
    return u.astype(np.uint32).view(np.float32)


def window_bin(key32) -> np.ndarray:
    """Bin of the 4096-bin window [~2^-31, 2.0]; -1 below it; keys above WTOP (NaN included) clamp into the top bin."""
    k16 = (np.asarray(key32, dtype=np.uint32) >> 16).astype(np.int64)
    return np.where(k16 < WBASE, -1, np.minimum(k16, WTOP) - WBASE)


def make_keys(scores, rows) -> np.ndarray:
    """score_key << 32 | row"""
    return (score_key(scores).astype(np.uint64) << np.uint64(32)) | np.asarray(rows, dtype=np.uint64)


def _next_pow2(v: int) -> int:
    p = 1
    while p < v:
        p <<= 1
    return p


def _emit(slots: int) -> str:
    return RANK if _next_pow2(max(int(slots), 2)) <= FINAL_THREADS else BITONIC


def _window_cut(bins: np.ndarray, k: int):
    """pick_bucket over the window histogram: (bin holding the k-th best from the top, keys at or above that bin), or
    (None, keys inside the window) when the window holds fewer than k."""
    inside = bins[bins >= 0]
    if inside.size < k:
        return None, int(inside.size)
    hist = np.bincount(inside, minlength=WBINS)
    from_top = np.cumsum(hist[::-1])                      # from_top[i]: keys in bins >= WBINS - 1 - i
    i = int(np.searchsorted(from_top, k, side="left"))    # first i with from_top[i] >= k
    return WBINS - 1 - i, int(from_top[i])


def _kth_largest_or_zero(values: np.ndarray, k: int) -> int:
    """block_kth_of_thread_values: the k-th largest of the values, 0 when fewer than k are non-zero."""
    nz = np.sort(values[values != 0])[::-1]
    return int(nz[k - 1]) if nz.size >= k else 0


# ---- run_select over a score vector -------------------------------------------------------------------
def route_scores(v, k: int) -> Route:
    v = np.asarray(v, dtype=np.float32)
    n = v.size
    count = min(int(k), n)
    if n <= SORT_CAP:
        return Route(D, _emit(n), None, None, n)
    if count > SEL_KMAX:
        return Route(B, None, None, None, None)
    keys = score_key(v)
    bstar, n_cand = _window_cut(window_bin(keys), count)
    if bstar is None:                                   # the filter sets the flag and appends nothing
        return Route(RAW_FLAG, _emit(count), 1, 0, count)
    if n_cand > CAND_CAP:
        return Route(RAW_OVERFLOW, _emit(count), 0, n_cand, count)
    if n_cand > FINAL_REG_MAX:
        return Route(CAND_RADIX, _emit(count), 0, n_cand, count)
    if n_cand <= FINAL_DIRECT:
        return Route(DIRECT, _emit(n_cand), 0, n_cand, n_cand)
    # Register route.  The filter appends in scheduling order, so which candidate sits in which thread is not known.
    if n_cand <= SORT_CAP:
        # every candidate is at or above bin b*, so the window pass keeps all of them and they fit the sort; the pivot of
        # the per-thread maxima (every thread holds >= 4 non-zero keys, so it exists) keeps at most all of them too
        if count <= FINAL_THREADS:
            return Route(MAXIMA, None, 0, n_cand, None)
        return Route(WINDOW, _emit(n_cand), 0, n_cand, n_cand)
    # n_cand > SORT_CAP: the window pass overflows the sort, so without the pivot the register radix select answers
    if count > FINAL_THREADS:
        return Route(REG_RADIX, _emit(count), 0, n_cand, count)
    # the pivot is at most the count-th best score: everything at or above THAT is at or above the pivot in any order
    cand = np.sort(keys[window_bin(keys) >= bstar])[::-1]
    if int(np.count_nonzero(cand >= cand[count - 1])) > SORT_CAP:
        return Route(REG_RADIX, _emit(count), 0, n_cand, count)
    return Route(UNDETERMINED, None, 0, n_cand, None)


def radix_exit_shift(keys, k: int) -> int:
    """The shift of the pass at which block_radix_select (11 bits per pass from bit 53, then the low 9 bits) returns for the
    k-th largest of the unique 64-bit keys: a pass returns early when the bucket it picked is selected whole.  0: the last
    pass ran."""
    keys = np.asarray(keys, dtype=np.uint64)
    k_rem = int(k)
    for shift in (53, 42, 31, 20, 9):
        bucket = ((keys >> np.uint64(shift)) & np.uint64(2047)).astype(np.int64)
        from_top = np.cumsum(np.bincount(bucket, minlength=2048)[::-1])
        i = int(np.searchsorted(from_top, k_rem, side="left"))
        b = 2047 - i
        in_bucket = int(from_top[i] - (from_top[i - 1] if i else 0))
        k_rem -= int(from_top[i - 1]) if i else 0
        if in_bucket == k_rem:
            return shift
        keys = keys[bucket == b]
    return 0


# ---- select_final_kernel mode 3 over a candidate list in a given order ------------------------------------
def live_keys(keys, n_cand: int, dead=None) -> np.ndarray:
    """The keys the kernel keeps: the first min(n_cand, len) of the list, those of masked rows struck out (0)."""
    keys = np.asarray(keys, dtype=np.uint64)[: min(int(n_cand), CAND_CAP)].copy()
    if dead is not None and keys.size:
        rows = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        keys[np.asarray(dead, dtype=bool)[rows]] = 0
    return keys


def route_candidates(keys, n_cand: int, count: int, dead=None) -> Route:
    """Exact: thread t of the final workgroup holds keys[t::256], so the pivot is known.  `dead`: bool per index row."""
    if n_cand > CAND_CAP:
        return Route(MARKED, None, 0, n_cand, None)
    kept = live_keys(keys, n_cand, dead)
    assert kept.size == n_cand, "a claim within the capacity needs that many keys"
    n_live = int(np.count_nonzero(kept))
    if n_live < count:
        return Route(MARKED, None, 0, n_cand, None)
    if n_cand <= FINAL_DIRECT:
        return Route(DIRECT, _emit(n_cand), 0, n_cand, n_cand)
    if n_cand > FINAL_REG_MAX:
        return Route(CAND_RADIX, _emit(count), 0, n_cand, count)
    sk = (kept >> np.uint64(32)).astype(np.uint32)      # the score halves; 0 for a struck-out key
    if count <= FINAL_THREADS:
        tmax = np.zeros(FINAL_THREADS, dtype=np.uint32)
        for t in range(FINAL_THREADS):
            mine = sk[t::FINAL_THREADS]
            tmax[t] = mine.max() if mine.size else 0
        pivot = _kth_largest_or_zero(tmax, count)
        if pivot != 0:
            total = int(np.count_nonzero(sk >= pivot))
            if total <= SORT_CAP:
                return Route(MAXIMA, _emit(total), 0, n_cand, total)
    bins = window_bin(sk)[kept != 0]
    bstar, total = _window_cut(bins, count)
    if bstar is not None and total <= SORT_CAP:
        return Route(WINDOW, _emit(total), 0, n_cand, total)
    return Route(REG_RADIX, _emit(count), 0, n_cand, count)


def expected_candidates(keys, n_cand: int, count: int, k: int, dead=None, row_offset: int = 0):
    """(score bits u32[k], rows i64[k]) the kernel must return: the live keys sorted descending, -inf / -1 past count;
    a marked query has -inf / -2 everywhere."""
    bits = np.full(k, np.float32(-np.inf).view(np.uint32), dtype=np.uint32)
    rows = np.full(k, -1, dtype=np.int64)
    if route_candidates(keys, n_cand, count, dead).name == MARKED:
        rows[:] = -2
        return bits, rows
    kept = live_keys(keys, n_cand, dead)
    top = np.sort(kept[kept != 0])[::-1][:count]
    bits[:count] = key_score((top >> np.uint64(32)).astype(np.uint32)).view(np.uint32)
    rows[:count] = (top & np.uint64(0xFFFFFFFF)).astype(np.int64) + row_offset
    return bits, rows


# ---- prefix_kth_kernel ------------------------------------------------------------------------------------
def route_kth(v, k: int, misaligned: bool = False) -> Route:
    v = np.asarray(v, dtype=np.float32)
    n = v.size
    assert 1 <= k <= n
    if n > PK_REG_MAX or misaligned:
        return Route(STREAM, None, None, None, None)
    keys = score_key(v)
    if k <= FINAL_THREADS:
        # thread t holds the float4 groups t, t + 256, ...: element i belongs to thread (i // 4) % 256
        owner = (np.arange(n) // 4) % FINAL_THREADS
        tmax = np.zeros(FINAL_THREADS, dtype=np.uint32)
        np.maximum.at(tmax, owner, keys)
        pivot = _kth_largest_or_zero(tmax, k)
        if pivot != 0:
            total = int(np.count_nonzero(keys >= pivot))
            if total <= PK_LIST:
                return Route(MAXIMA, None, None, None, total)
    bins = window_bin(keys)
    bstar, _ = _window_cut(bins, k)
    if bstar is not None:
        total = int(np.count_nonzero(bins == bstar))
        if total <= PK_LIST:
            return Route(WINDOW, None, None, None, total)
    return Route(REG_RADIX, None, None, None, None)


def expected_kth_bits(v, k: int) -> int:
    """Bits of the k-th largest score as key_score returns it (-0 as +0, NaN canonical)."""
    keys = np.sort(score_key(v))[::-1]
    return int(key_score(keys[k - 1: k]).view(np.uint32)[0])


def expected_scores(v, k: int, row_offset: int = 0):
    """(score bits u32[k], rows i64[k]) of run_select over v: oracle.total_order_top_k's rows, the scores as key_score
    returns them, -inf / -1 past min(k, n)."""
    from oracle import svs_oracle as oracle
    v = np.asarray(v, dtype=np.float32)
    top = oracle.total_order_top_k(v, k)
    bits = np.full(k, np.float32(-np.inf).view(np.uint32), dtype=np.uint32)
    rows = np.full(k, -1, dtype=np.int64)
    r = np.array([i for _, i in top], dtype=np.int64)
    bits[: r.size] = key_score(score_key(v[r])).view(np.uint32)
    rows[: r.size] = r + row_offset
    return bits, rows

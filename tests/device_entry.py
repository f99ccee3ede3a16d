"""Helpers of tests/test_device_batch_gpu.py: buffers for svs_index_search_device that show what the call touched, and
the f64 oracle of a batched search.  Plain numpy at import time: torch is handed in by the tests that have a device.

  * Outputs: scores / rows of one call, pre-filled with sentinels (NaN / -7), with GUARD elements of the same sentinels
    in front of and behind the nq * k the call owns; read() asserts the guards and returns the (nq, k) arrays.
  * QueryBuf: the nq * d query floats as a view into a larger tensor whose other floats are NaN -- a kernel that reads
    outside the view computes NaN scores -- at a chosen offset (in floats) from a 16-byte boundary.
  * check_topk: entries [0, count) of every query against the f64 oracle on the live stored rows (assert_topk_parity,
    rows mapped through the live list), entries [count, k) exactly -inf / -1.
"""
import numpy as np

from compare import assert_topk_parity
from oracle import svs_oracle as oracle

GUARD = 64            # sentinel elements on either side of an output
SENTINEL_ROW = -7
PAD = 256             # NaN floats on either side of a query view (a multiple of 4: the view keeps the offset asked for)


class Outputs:
    def __init__(self, torch, dev, nq, k):
        self.nq, self.k = nq, k
        self.s_all = torch.full((2 * GUARD + nq * k,), float("nan"), device=dev, dtype=torch.float32)
        self.r_all = torch.full((2 * GUARD + nq * k,), SENTINEL_ROW, device=dev, dtype=torch.int64)
        self.s, self.r = self.s_all[GUARD:GUARD + nq * k], self.r_all[GUARD:GUARD + nq * k]

    @property
    def ptrs(self):
        return self.s.data_ptr(), self.r.data_ptr()

    def host(self, s_all=None, r_all=None):
        """(scores f32 (nq, k), rows i64 (nq, k)) of this buffer -- or of a device copy of it -- guards asserted."""
        s = (self.s_all if s_all is None else s_all).cpu().numpy()
        r = (self.r_all if r_all is None else r_all).cpu().numpy()
        for g in (s[:GUARD], s[s.size - GUARD:]):
            assert np.isnan(g).all(), "a score guard was written"
        for g in (r[:GUARD], r[r.size - GUARD:]):
            assert (g == SENTINEL_ROW).all(), "a row guard was written"
        return s[GUARD:s.size - GUARD].reshape(self.nq, self.k).copy(), r[GUARD:r.size - GUARD].reshape(self.nq, self.k).copy()

    def untouched(self):
        s, r = self.host()
        return bool(np.isnan(s).all() and (r == SENTINEL_ROW).all())


class QueryBuf:
    def __init__(self, torch, dev, q, offset=0, fill=True):
        """q: numpy f32 (nq, d).  offset: floats past a 16-byte boundary at which the view starts.  fill=False leaves the
        view NaN as well (a producer on some stream writes it later: src holds the queries)."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        self.nq, self.d = q.shape
        self.all = torch.full((2 * PAD + 4 + q.size,), float("nan"), device=dev, dtype=torch.float32)
        assert self.all.data_ptr() % 16 == 0
        self.view = self.all[PAD + offset:PAD + offset + q.size]
        assert self.view.data_ptr() % 16 == 4 * (offset % 4)
        self.src = torch.from_numpy(q.reshape(-1)).to(dev)
        if fill:
            self.view.copy_(self.src)

    @property
    def ptr(self):
        return self.view.data_ptr()


def search_device(idx, qb, k, out, stream, ahead=False, ready=None):
    """One svs_index_search_device(_ahead) call of all of qb's queries into out; no synchronisation.  -> count"""
    s_ptr, r_ptr = out.ptrs
    if ahead:
        return idx.search_device_ahead(qb.ptr, qb.nq, qb.d, k, s_ptr, r_ptr, stream.cuda_stream, ready_event=ready)
    return idx.search_device(qb.ptr, qb.nq, qb.d, k, s_ptr, r_ptr, stream.cuda_stream)


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)


def same_bits(got, exp, label=""):
    """rows equal, scores equal as uint32"""
    (gs, gr), (es, er) = got, exp
    assert gr.shape == er.shape and gs.shape == es.shape, (label, gr.shape, er.shape)
    assert np.array_equal(gr, er), (label, "rows", np.argwhere(gr != er)[:8].tolist())
    assert np.array_equal(bits(gs), bits(es)), (label, "scores", np.argwhere(bits(gs) != bits(es))[:8].tolist())


def f64_scores(md, qd):
    """(nq, n) = qd @ md.T accumulated in f64"""
    return qd.astype(np.float64) @ md.astype(np.float64).T


def check_topk(s, r, count, md, qd, label, dead=None, row_offset=0, queries=None):
    """s, r: (nq, k) as the device entry wrote them.  md: the stored rows (all n of them), qd: the stored queries,
    dead: masked LOCAL rows.  Entries [0, count) of every query (or of `queries`) against the oracle on the live rows;
    entries [count, k) are -inf / -1 exactly; no masked row comes back.  -> largest |score - f64| seen."""
    n = md.shape[0]
    nq, k = s.shape
    live = np.arange(n) if dead is None or not len(dead) else np.setdiff1d(np.arange(n), dead)
    assert count == min(k, live.size), f"{label}: count {count}, live rows {live.size}, k {k}"
    assert np.all(np.isneginf(s[:, count:])), f"{label}: scores past count are not -inf: {s[:, count:][~np.isneginf(s[:, count:])][:8]}"
    assert np.all(r[:, count:] == -1), f"{label}: rows past count are not -1: {r[:, count:][r[:, count:] != -1][:8]}"
    worst = 0.0
    ml = md[live]
    for q in (range(nq) if queries is None else queries):
        assert not np.isnan(s[q, :count]).any(), f"{label} q{q}: NaN scores (a read outside the queries, or an entry nobody wrote)"
        loc = r[q, :count] - row_offset
        assert loc.min(initial=0) >= 0 and loc.max(initial=0) < n, f"{label} q{q}: rows outside the index: {r[q, :count][:8]}"
        if dead is not None and len(dead):
            assert not np.isin(loc, dead).any(), f"{label} q{q}: a masked row came back"
        truth = np.full(n, -np.inf)
        truth[live] = f64_scores(ml, qd[q:q + 1])[0]
        exp = oracle.cpu_top_k(np.dot(ml, qd[q]), count)
        assert_topk_parity(s[q, :count], loc, [x for x, _ in exp], [int(live[i]) for _, i in exp], truth, label=f"{label} q{q}")
        if count:
            worst = max(worst, float(np.abs(s[q, :count].astype(np.float64) - truth[loc]).max()))
    return worst

#!/usr/bin/env python3
"""Collapsed search (svs_index_search_collapsed): host-call time of DeviceIndex.search_batch_collapsed for ONE query,
k = 100, zero="single", over a 1M x 1536 corpus built on the device, for four group layouts of column 1
  own      every row its own value (the table at its fullest: 1M groups)
  adj8     runs of 8 adjacent rows
  scat8    groups of 8 rows scattered over the corpus (r mod n/8)
  half     ONE group holding every second row, every other row its own value
beside -- in the same process and session, alternating call by call (an untimed call behind every (b): the GPU idles
while numpy works) --
  (a) above     DeviceIndex.search_batch_above, count only, cut-off at the 100th best score: the pass every such entry
                pays (one score pass plus one filter over the score vector),
  (b) numpy     DeviceIndex.scores + grouping in numpy over a host copy of the column: what a caller can do without the
                entry, exactly,
  (c) overfetch DeviceIndex.search_batch with n = 2k, 4k, ... until k distinct values appear among the rows: what callers
                do today (exact only when the loop ends before n runs out of rows of repeated groups; its answer is
                checked against the entry's).
The answers are checked to agree.  Then, with svs_index_set_timing on, the split of the call between its stages from the
HIP events around them (svs_internal_collapse_kernel_ms): reduce kernel, mark kernel, the table's fill, the top-k stage.
Writes a table and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call, and the ratios.
  usage: collapse_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=40] [out=profiles/collapse_time.txt]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from svs_amd import DeviceIndex, _native
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 40
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "collapse_time.txt")
K = 100
COLUMN = 1
LAYOUTS = ["own", "adj8", "scat8", "half"]
STAGES = ["reduce", "mark", "clear", "select"]
lib = _native.load()


def column_of(layout):
    r = np.arange(n, dtype=np.int64)
    if layout == "own":
        v = r + 1
    elif layout == "adj8":
        v = r // 8 + 1
    elif layout == "scat8":
        v = r % max(n // 8, 1) + 1
    else:
        v = np.where(r % 2 == 0, n + 7, r + 1)
    return v.astype(np.uint32)


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def collapsed(idx, q):
    s, r, v, counts, groups = idx.search_batch_collapsed(q, K, COLUMN, "single")
    c = int(counts[0])
    return s[0, :c], r[0, :c], v[0, :c], int(groups[0])


def numpy_group_by(idx, q, col):
    s = idx.scores(q)
    order = np.lexsort((np.arange(n), s, col))                      # by value, then score, then row
    last = np.nonzero(np.append(col[order][1:] != col[order][:-1], True))[0]
    best = order[last]                                              # (the layouts hold no 0: no exempt rows)
    rank = np.lexsort((best, s[best]))[::-1][:K]
    return s[best[rank]], best[rank], col[best[rank]], len(best)


def overfetch(idx, q, col):
    fetch = 2 * K
    while True:
        s, r = idx.search_batch(q, fetch)
        vals = col[r[0]]
        _, first = np.unique(vals, return_index=True)               # rows come best first: a value's first row is its best
        if len(first) >= K or fetch >= n:
            keep = np.sort(first)[:K]
            return s[0][keep], r[0][keep], vals[keep], fetch
        fetch = min(2 * fetch, n)


def stats(v):
    q25, q50, q75 = np.percentile(v, [25, 50, 75])
    return {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(16)
out = {"n": n, "d": d, "k": K, "csrc_sha16": csrc_sha16(), "reps": reps}
lines, split_lines = [], []
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    q = torch.randn((1, d), device=dev, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    cut = np.sort(idx.scores(q[0]))[::-1][K - 1]
    res = {}
    for layout in LAYOUTS:
        col = column_of(layout)
        idx.set_column(COLUMN, col)
        # (b) keeps the host busy for a long time while the GPU idles, and the call behind such a pause is slower
        # whatever it is: (b) goes first and an untimed call follows it
        calls = {"numpy_group_by": lambda: numpy_group_by(idx, q[0], col),
                 "(untimed)": lambda: idx.search_batch_above(q, [cut], 0),
                 "collapsed": lambda: collapsed(idx, q),
                 "above_count": lambda: idx.search_batch_above(q, [cut], 0),
                 "overfetch": lambda: overfetch(idx, q, col)}
        # the three agree (and the calls are warm afterwards)
        es, er, ev, eg = numpy_group_by(idx, q[0], col)
        s, r, v, groups = collapsed(idx, q)
        assert groups == eg and r.tolist() == er.tolist() and v.tolist() == ev.tolist() and s.tolist() == es.tolist(), (dtype, layout)
        os_, or_, ov, fetched = overfetch(idx, q, col)
        over_ok = or_.tolist() == er.tolist() and ov.tolist() == ev.tolist()   # (recorded, not asserted: the loop is the callers' heuristic)
        b_reps = max(3, reps // 8)                                   # (b) sorts n rows on the host: a few runs are enough
        times = {name: [] for name in calls}
        for i in range(reps):       # alternating, so that drift hits all alike
            for name, fn in calls.items():
                if name == "numpy_group_by" and i >= b_reps:
                    continue
                times[name].append(timed(fn))
        r_ = {name: stats(t) for name, t in times.items() if name != "(untimed)"}
        # the split, from the events around the stages (their own calls: the events cost a little)
        idx.set_timing(1)
        ms = (C.c_double * 4)()
        parts = [[] for _ in STAGES]
        for _ in range(reps):
            collapsed(idx, q)
            _native.check(lib.svs_internal_collapse_kernel_ms(ms))
            for i in range(4):
                parts[i].append(ms[i])
        idx.set_timing(0)
        split = {st: round(float(np.median(p)), 4) for st, p in zip(STAGES, parts)}
        a, fl, np_, of = (r_[k]["p50_ms"] for k in ("collapsed", "above_count", "numpy_group_by", "overfetch"))
        r_.update(groups=int(groups), overfetch_rows=int(fetched), overfetch_agrees=bool(over_ok), split_ms=split, ratio_to_above=round(a / fl, 3),
                  numpy_over_collapsed=round(np_ / a, 2), overfetch_over_collapsed=round(of / a, 3))
        res[layout] = r_
        lines.append(f"{dtype:5s} {layout:6s} {int(groups):9d} {a:9.4f} {r_['collapsed']['spread_ms']:8.4f} {fl:9.4f} {np_:10.4f} {of:9.4f} {int(fetched):8d} "
                     f"{a / fl:7.3f} {np_ / a:8.2f} {of / a:8.3f}")
        split_lines.append(f"{dtype:5s} {layout:6s} " + " ".join(f"{split[st]:8.4f}" for st in STAGES) + f" {sum(split.values()):8.4f}")
        print(f"[collapse_time] {lines[-1]} | {split_lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Collapsed search: DeviceIndex.search_batch_collapsed (one query, k = 100, column 1, zero = single) against (a) search_batch_above, count only,",
    "cut-off at the 100th best score, (b) DeviceIndex.scores + grouping in numpy over a host copy of the column and (c) the over-fetch loop on",
    "search_batch (n = 2k, 4k, ... until k distinct values) (tools/collapse_time.py, MI355X, one process, the calls alternating call by call,",
    "one untimed call behind every (b)).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls ((b): of {max(3, reps // 8)}), csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the collapsed calls.  times in ms.  layout own: every row its own value; adj8: runs of 8 adjacent rows;",
    "scat8: groups of 8 rows scattered by r mod n/8; half: one group holds every second row, the other rows their own value.",
    "fetched = the n the over-fetch loop ended with.  /(a): collapsed over (a); (b)/, (c)/: (b) and (c) over collapsed.",
    "",
    f"{'dtype':5s} {'layout':6s} {'groups':>9s} {'collapsed':>9s} {'(spread)':>8s} {'(a) above':>9s} {'(b) numpy':>10s} {'(c) over':>9s} {'fetched':>8s} "
    f"{'/(a)':>7s} {'(b)/':>8s} {'(c)/':>8s}",
]
mid = ["", "The stages of the call's one query, from the HIP events around them (svs_index_set_timing on; median of the same number of calls, ms):",
       f"{'dtype':5s} {'layout':6s} " + " ".join(f"{st:>8s}" for st in STAGES) + f" {'sum':>8s}"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines + mid + split_lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

#!/usr/bin/env python3
"""Collapsed search under a predicate (svs_index_search_collapsed_where): host-call time of
DeviceIndex.search_batch_collapsed_where for ONE query, k = 100, zero="single", over a 1M x 1536 corpus built on the
device.  Column 1 holds the groups (runs of 8 adjacent rows), column 0 a scattered number 0 .. 99 per row, and the
predicate ``(0, "range", (0, p - 1))`` admits p = 1, 10, 50 and 100 percent of the rows.  Beside the call -- in the same
process and session, alternating call by call (an untimed call behind every (b): the GPU idles while numpy works) --
  (a) where      DeviceIndex.search_batch_where with the same predicate and k = 100: the floor -- the same filter and
                 the same gathered bytes, no grouping,
  (b) numpy      DeviceIndex.search_batch_where with k = matched plus a numpy group-by over the read-back: what a caller
                 can do exactly without the entry; its answer is asserted equal to the entry's,
  (c) unscoped   DeviceIndex.search_batch_collapsed over the whole corpus: ANOTHER answer (no predicate), shown only as
                 the cost of a full pass.
Then, with svs_index_set_timing on, the split of the call between its stages from the HIP events around them
(svs_internal_collapse_scope_kernel_ms): filter (count, scan and write), gather, reduce, mark, the table's fill, the
top-k stage.  Writes a table and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call, the
call minus (a), and the ratios.
  usage: collapse_where_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=30] [out=profiles/collapse_where_time.txt]"""
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "collapse_where_time.txt")
K = 100
SCOPE_COLUMN, GROUP_COLUMN = 0, 1
PERCENTS = [1, 10, 50, 100]
STAGES = ["filter", "gather", "reduce", "mark", "clear", "select"]
lib = _native.load()


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def scoped(idx, q, where):
    s, r, v, counts, groups, matched = idx.search_batch_collapsed_where(q, K, where, GROUP_COLUMN, "single")
    c = int(counts[0])
    return s[0, :c], r[0, :c], v[0, :c], int(groups[0]), matched


def numpy_group_by(idx, q, where, matched, col):
    s, r, _ = idx.search_batch_where(q, matched, where)              # every matching row, best first
    s, r = s[0], r[0]
    vals = col[r]
    _, first = np.unique(vals, return_index=True)                    # a value's first row is its best (the values hold no 0)
    keep = np.sort(first)
    return s[keep][:K], r[keep][:K], vals[keep][:K], len(keep)


def stats(v):
    q25, q50, q75 = np.percentile(v, [25, 50, 75])
    return {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(16)
out = {"n": n, "d": d, "k": K, "csrc_sha16": csrc_sha16(), "reps": reps}
lines, split_lines = [], []
rows_ = np.arange(n, dtype=np.uint64)
scope_col = (((rows_ * np.uint64(2654435761)) % np.uint64(1 << 32)) >> np.uint64(16)) % np.uint64(100)
scope_col = scope_col.astype(np.uint32)
group_col = (np.arange(n, dtype=np.int64) // 8 + 1).astype(np.uint32)
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
    idx.set_column(SCOPE_COLUMN, scope_col)
    idx.set_column(GROUP_COLUMN, group_col)
    res = {}
    for pct in PERCENTS:
        where = [(SCOPE_COLUMN, "range", (0, pct - 1))]
        matched = idx.count_where(where)
        # (b) keeps the host busy while the GPU idles, and the call behind such a pause is slower whatever it is: (b)
        # goes first and an untimed call follows it
        calls = {"numpy_group_by": lambda: numpy_group_by(idx, q, where, matched, group_col),
                 "(untimed)": lambda: idx.search_batch_where(q, K, where),
                 "scoped": lambda: scoped(idx, q, where),
                 "where_k100": lambda: idx.search_batch_where(q, K, where),
                 "unscoped": lambda: idx.search_batch_collapsed(q, K, GROUP_COLUMN, "single")}
        # (b) and the entry agree (and the calls are warm afterwards)
        es, er, ev, eg = numpy_group_by(idx, q, where, matched, group_col)
        s, r, v, groups, m = scoped(idx, q, where)
        assert m == matched and groups == eg and r.tolist() == er.tolist() and v.tolist() == ev.tolist(), (dtype, pct)
        assert s.tobytes() == es.tobytes(), (dtype, pct)
        idx.search_batch_collapsed(q, K, GROUP_COLUMN, "single")
        b_reps = max(3, reps // 6)                                   # (b) sorts up to n rows: a few runs are enough
        times = {name: [] for name in calls}
        for i in range(reps):       # alternating, so that drift hits all alike
            for name, fn in calls.items():
                if name == "numpy_group_by" and i >= b_reps:
                    continue
                times[name].append(timed(fn))
        r_ = {name: stats(t) for name, t in times.items() if name != "(untimed)"}
        # the split, from the events around the stages (their own calls: the events cost a little)
        idx.set_timing(1)
        ms = (C.c_double * len(STAGES))()
        parts = [[] for _ in STAGES]
        for _ in range(reps):
            scoped(idx, q, where)
            _native.check(lib.svs_internal_collapse_scope_kernel_ms(ms))
            for i in range(len(STAGES)):
                parts[i].append(ms[i])
        idx.set_timing(0)
        split = {st: round(float(np.median(p)), 4) for st, p in zip(STAGES, parts)}
        a, fl, np_, un = (r_[k]["p50_ms"] for k in ("scoped", "where_k100", "numpy_group_by", "unscoped"))
        r_.update(matched=int(matched), groups=int(groups), split_ms=split, minus_where_ms=round(a - fl, 4), numpy_over_scoped=round(np_ / a, 2),
                  scoped_over_unscoped=round(a / un, 3))
        res[f"{pct}%"] = r_
        lines.append(f"{dtype:5s} {pct:4d}% {int(matched):9d} {int(groups):9d} {a:9.4f} {r_['scoped']['spread_ms']:8.4f} {fl:9.4f} {np_:10.4f} {un:9.4f} "
                     f"{a - fl:8.4f} {np_ / a:8.2f} {a / un:8.3f}")
        split_lines.append(f"{dtype:5s} {pct:4d}% " + " ".join(f"{split[st]:8.4f}" for st in STAGES) + f" {sum(split.values()):8.4f}")
        print(f"[collapse_where_time] {lines[-1]} | {split_lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Collapsed search under a predicate: DeviceIndex.search_batch_collapsed_where (one query, k = 100, groups of 8 adjacent rows in column 1,",
    "zero = single, predicate (0, range, (0, p - 1)) over a scattered column of 0 .. 99) against (a) search_batch_where with the same predicate",
    "and k = 100, (b) search_batch_where with k = matched + a numpy group-by over the read-back (its answer is asserted equal) and (c) the",
    "unscoped search_batch_collapsed over the whole corpus (another answer: the cost of a full pass)",
    "(tools/collapse_where_time.py, MI355X, one process, the calls alternating call by call, one untimed call behind every (b)).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls ((b): of {max(3, reps // 6)}), csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the scoped calls.  times in ms.  -(a): scoped minus (a), what grouping `matched` rows costs;",
    "(b)/: (b) over scoped; /(c): scoped over (c).",
    "",
    f"{'dtype':5s} {'scope':>5s} {'matched':>9s} {'groups':>9s} {'scoped':>9s} {'(spread)':>8s} {'(a) where':>9s} {'(b) numpy':>10s} {'(c) full':>9s} "
    f"{'-(a)':>8s} {'(b)/':>8s} {'/(c)':>8s}",
]
mid = ["", "The stages of the call, from the HIP events around them (svs_index_set_timing on; median of the same number of calls, ms):",
       f"{'dtype':5s} {'scope':>5s} " + " ".join(f"{st:>8s}" for st in STAGES) + f" {'sum':>8s}"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines + mid + split_lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

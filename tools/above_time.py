#!/usr/bin/env python3
"""Threshold search (svs_index_search_above): host-call time of DeviceIndex.search_batch_above for ONE query over a
1M x 1536 corpus built on the device, beside -- in the same process, alternating call by call --
  (b) top-k   DeviceIndex.search_batch with k = 100 under variant 11 (never screened): the same score pass, and
  (c) numpy   DeviceIndex.scores + the numpy filter and ordering: what a caller has to do without the entry.
(a) is taken at cut-offs giving totals of 0, 100, 4,000 and 40,000 rows with limit = 100 (the last one overflows the
candidate list and is re-run through the exact top-k stage), and at total 100 with limit = 0 (count only).  Writes a
table and one JSON line: per dtype the p50 in ms and the 25th-75th percentile spread of every call.
  usage: above_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=40] [out=profiles/above_time.txt]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from svs_amd import DeviceIndex
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 40
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "above_time.txt")
LIMIT = 100
TOTALS = [0, 100, 4000, 40000]


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def numpy_filter(idx, q, cut, limit):
    s = idx.scores(q)
    rows = np.nonzero(s >= cut)[0]
    order = np.lexsort((rows, s[rows]))[::-1][:limit]
    return s[rows[order]], rows[order], len(rows)


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(14)
out = {"n": n, "d": d, "limit": LIMIT, "csrc_sha16": csrc_sha16(), "reps": reps}
lines = []
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    idx.set_variant(11)   # (b) unscreened, as (a) always is: the same score kernel in all three
    q = torch.randn((1, d), device=dev, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    ranked = np.sort(idx.scores(q[0]))[::-1]
    cuts = {t: (np.float32(2.0) if t == 0 else ranked[t - 1]) for t in TOTALS}
    calls = {f"above_total_{t}": (lambda c=cuts[t]: idx.search_batch_above(q, [c], LIMIT)) for t in TOTALS}
    calls["above_count_only_100"] = lambda: idx.search_batch_above(q, [cuts[100]], 0)
    calls["topk_100"] = lambda: idx.search_batch(q, LIMIT)
    calls["numpy_filter_100"] = lambda: numpy_filter(idx, q[0], cuts[100], LIMIT)
    for t in TOTALS:      # the three agree (and the calls are warm afterwards)
        s, r, total = idx.search_batch_above(q, [cuts[t]], LIMIT)[0]
        es, er, etotal = numpy_filter(idx, q[0], cuts[t], LIMIT)
        assert total == etotal and r.tolist() == er.tolist() and s.tolist() == es.tolist(), (dtype, t)
    for fn in calls.values():
        fn()
    times = {name: [] for name in calls}
    for _ in range(reps):       # alternating, so that drift hits all alike
        for name, fn in calls.items():
            times[name].append(timed(fn))
    res = {}
    for name, v in times.items():
        q25, q50, q75 = np.percentile(v, [25, 50, 75])
        res[name] = {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}
        lines.append(f"{dtype:5s} {name:22s} {q50:9.4f} {q75 - q25:9.4f}")
        print(f"[above_time] {dtype} {name}: {res[name]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Threshold search: DeviceIndex.search_batch_above (one query, limit = 100) against the top-100 search under variant 11 (the same",
    "unscreened score pass) and against DeviceIndex.scores + a numpy filter (tools/above_time.py, MI355X, one process, the calls",
    "alternating call by call).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls, csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the calls.  times in ms.  above_total_40000 overflows the candidate list: it is re-run",
    "through the exact top-k stage (a second score pass).",
    "",
    f"{'dtype':5s} {'call':22s} {'p50':>9s} {'(spread)':>9s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

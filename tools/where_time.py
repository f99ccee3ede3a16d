#!/usr/bin/env python3
"""Predicate search (svs_index_search_where): host-call time of ONE query, k = 100, over a 1M x 1536 f32 corpus built on
the device whose column 0 carries labels 1 .. 4 (1 %, 9 %, 40 % and 50 % of the rows), for selections of about 1 %,
10 % and 50 % of the rows through four forms -- in the same process, alternating call by call:
  (a) labeled   DeviceIndex.search_batch_labeled with the sets {1}, {1,2}, {1,2,3};
  (b) where1    DeviceIndex.search_batch_where with the same ONE IN term on column 0;
  (c) where4    DeviceIndex.search_batch_where with FOUR terms over four columns that select the same rows: the IN term on
                column 0, and a RANGE on column 1, an ANY_BITS on column 2 and a NOT IN on column 3 that every row
                satisfies -- four column loads per row instead of one;
  (d) rows      DeviceIndex.search_batch_within over the SAME rows given as a ready-made ascending int64 host list.
Every form is timed twice under two names (``..._x`` and ``..._y``), so that the file shows the run-to-run spread of one
and the same call beside the differences between the forms.
The host_* rows are Python alone, nothing launched: what the wrapper does to its filter argument before the native call --
``labels_u32(set)`` for (a), ``pack_where(where)`` (checking, sorting and the C array of terms) for (b) and (c).
Writes a table and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call.
  usage: where_time.py [n=1000000] [d=1536] [reps=40] [out=profiles/where_time.txt]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from svs_amd import DeviceIndex
from svs_amd.index import labels_u32, pack_where
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 40
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "where_time.txt")
K = 100
SETS = {"1pct": [1], "10pct": [1, 2], "50pct": [1, 2, 3]}


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(15)
out = {"n": n, "d": d, "k": K, "csrc_sha16": csrc_sha16(), "reps": reps}
lines = []
rng = np.random.default_rng(16)
u = rng.random(n)
labels = np.select([u < 0.01, u < 0.10, u < 0.50], [1, 2, 3], default=4).astype(np.uint32)
col1 = rng.integers(0, 1000, n).astype(np.uint32)                 # RANGE (0, 999): every row
col2 = (rng.integers(0, 1 << 20, n).astype(np.uint32) << 1) | 1   # ANY_BITS 1: every row
col3 = rng.integers(1, 1 << 31, n).astype(np.uint32)              # NOT IN {0}: every row
idx = DeviceIndex.empty(d, device=0, dtype="f32", reserve=n)
for r0 in range(0, n, 250_000):
    rows = min(250_000, n - r0)
    v = torch.randn((rows, d), device=dev, generator=g)
    v /= v.norm(dim=1, keepdim=True)
    idx.append_device(v.contiguous().data_ptr(), rows)
    del v
torch.cuda.synchronize()
idx.set_labels(labels)
for c, col in ((1, col1), (2, col2), (3, col3)):
    idx.set_column(c, col)
q = torch.randn((1, d), device=dev, generator=g)
q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
lists = {name: np.flatnonzero(np.isin(labels, s)).astype(np.int64) for name, s in SETS.items()}


def four(s):
    return [(0, "in", s), (1, "range", (0, 999)), (2, "any_bits", 1), (3, "not in", [0])]


calls = {}
for rep in ("x", "y"):
    for name, s in SETS.items():
        calls[f"labeled_{name}_{rep}"] = lambda s=s: idx.search_batch_labeled(q, K, s)
        calls[f"where1_{name}_{rep}"] = lambda s=s: idx.search_batch_where(q, K, [(0, "in", s)])
        calls[f"where4_{name}_{rep}"] = lambda s=s: idx.search_batch_where(q, K, four(s))
        calls[f"rows_{name}_{rep}"] = lambda r=lists[name]: idx.search_batch_within(q, K, r)
    calls[f"host_labels_u32_{rep}"] = lambda: labels_u32(SETS["10pct"])
    calls[f"host_pack_where1_{rep}"] = lambda: pack_where([(0, "in", SETS["10pct"])])
    calls[f"host_pack_where4_{rep}"] = lambda: pack_where(four(SETS["10pct"]))
calls["where4_count_only_10pct"] = lambda: idx.count_where(four(SETS["10pct"]))
calls["where1_count_only_10pct"] = lambda: idx.count_where([(0, "in", SETS["10pct"])])
for name, s in SETS.items():      # the four agree (and the calls are warm afterwards)
    a_s, a_r, matched = idx.search_batch_labeled(q, K, s)
    d_s, d_r = idx.search_batch_within(q, K, lists[name])
    for where in ([(0, "in", s)], four(s)):
        b_s, b_r, b_matched = idx.search_batch_where(q, K, where)
        assert b_matched == matched == len(lists[name]), (name, where)
        assert b_r.tolist() == a_r.tolist() == d_r.tolist() and b_s.tobytes() == a_s.tobytes() == d_s.tobytes(), (name, where)
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
    lines.append(f"{name:28s} {q50:9.4f} {q75 - q25:9.4f}")
    print(f"[where_time] {name}: {res[name]}", file=sys.stderr, flush=True)
res["matched"] = {name: int(len(r)) for name, r in lists.items()}
out["f32"] = res
idx.release()

head = [
    "Predicate search: DeviceIndex.search_batch_where (one query, k = 100; the filter on the device) with ONE IN term on",
    "column 0 (where1) and with FOUR terms over four columns selecting the same rows (where4), against",
    "DeviceIndex.search_batch_labeled with the same set (labeled) and DeviceIndex.search_batch_within over the same rows as a",
    "ready-made ascending host list (rows) (tools/where_time.py, MI355X, one process, the calls alternating call by call;",
    "_x and _y are the same call timed twice: their difference is the run-to-run spread).  host_* rows: the Python wrapper's",
    "work on its filter argument alone (the 10 % set), nothing launched.",
    f"n = {n}, d = {d}, f32, p50 of {reps} warmed calls, csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the calls.  times in ms.",
    "",
    f"{'call':28s} {'p50':>9s} {'(spread)':>9s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

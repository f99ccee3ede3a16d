#!/usr/bin/env python3
"""Labelled search (svs_index_search_labeled): host-call time of ONE query, k = 100, over a 1M x 1536 corpus built on the
device whose rows carry labels 1 .. 4 (1 %, 9 %, 40 % and 50 % of the rows), beside -- in the same process, alternating
call by call --
  (a) labeled   DeviceIndex.search_batch_labeled with the sets {1}, {1,2}, {1,2,3}, {1,2,3,4}: about 1 %, 10 %, 50 % and
                100 % of the rows; the filter runs on the device, and
  (b) rows      DeviceIndex.search_batch_within over the SAME rows given as a prebuilt ascending int64 host list (the
                list's construction is not timed): validation, u32 conversion and upload per call.
Then (c), on an on-disk KB of 100k docs on three levels (1 %, 9 %, 90 % of the docs): KB.retrieve_at_level against
KB.retrieve_within with the level's doc ids (the id list is prebuilt; its SQL and row mapping are part of the call).
Writes a table and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call.
  usage: labels_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=40] [kb_docs=100000] [kb_d=384] [out=profiles/labels_time.txt]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import svs_amd
from svs_amd import DeviceIndex
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 40
kb_docs = int(sys.argv[5]) if len(sys.argv) > 5 else 100_000
kb_d = int(sys.argv[6]) if len(sys.argv) > 6 else 384
out_path = sys.argv[7] if len(sys.argv) > 7 else os.path.join(ROOT, "profiles", "labels_time.txt")
K = 100
SETS = {"1pct": [1], "10pct": [1, 2], "50pct": [1, 2, 3], "100pct": [1, 2, 3, 4]}


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def run_alternating(calls, tag):
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
        lines.append(f"{tag:5s} {name:26s} {q50:9.4f} {q75 - q25:9.4f}")
        print(f"[labels_time] {tag} {name}: {res[name]}", file=sys.stderr, flush=True)
    return res


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(15)
out = {"n": n, "d": d, "k": K, "csrc_sha16": csrc_sha16(), "reps": reps}
lines = []
u = np.random.default_rng(16).random(n)
labels = np.select([u < 0.01, u < 0.10, u < 0.50], [1, 2, 3], default=4).astype(np.uint32)
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    idx.set_labels(labels)
    q = torch.randn((1, d), device=dev, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    lists = {name: np.flatnonzero(np.isin(labels, s)).astype(np.int64) for name, s in SETS.items()}
    calls = {}
    for name, s in SETS.items():
        calls[f"labeled_{name}"] = lambda s=s: idx.search_batch_labeled(q, K, s)
        calls[f"rows_{name}"] = lambda r=lists[name]: idx.search_batch_within(q, K, r)
    calls["labeled_count_only_10pct"] = lambda: idx.search_batch_labeled(q, 0, SETS["10pct"])
    for name, s in SETS.items():      # the two agree (and the calls are warm afterwards)
        a_s, a_r, matched = idx.search_batch_labeled(q, K, s)
        b_s, b_r = idx.search_batch_within(q, K, lists[name])
        assert matched == len(lists[name]) and a_r.tolist() == b_r.tolist() and a_s.tobytes() == b_s.tobytes(), (dtype, name)
    res = run_alternating(calls, dtype)
    res["matched"] = {name: int(len(r)) for name, r in lists.items()}
    out[dtype] = res
    idx.release()

# (c) the KB layer: one level named in the query against the level's doc ids handed over as a list
if kb_docs > 0:
    rng = np.random.default_rng(17)

    async def ef(texts):
        v = rng.standard_normal((len(texts), kb_d))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32).tolist()

    with tempfile.TemporaryDirectory() as tmp:
        kb = svs_amd.KB(os.path.join(tmp, "kb.sqlite"), ef)
        t0 = time.perf_counter()
        level_ids = {0: [], 1: [], 2: []}
        n_roots = max(kb_docs // 100, 1)
        with kb.bulk_add_docs() as add_doc:
            for r in range(n_roots):
                root = add_doc(f"r{r}")
                level_ids[0].append(root)
                for c in range(9):
                    child = add_doc(f"r{r}c{c}", parent_id=root)
                    level_ids[1].append(child)
                    for leaf in range(10):
                        level_ids[2].append(add_doc(f"r{r}c{c}l{leaf}", parent_id=child))
        kb.load()
        print(f"[labels_time] KB of {sum(map(len, level_ids.values()))} docs built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        calls = {}
        for lv in (0, 1, 2):
            calls[f"retrieve_at_level_{lv}"] = lambda lv=lv: kb.retrieve_at_level("a query", K, lv)
            calls[f"retrieve_within_level_{lv}"] = lambda lv=lv: kb.retrieve_within("a query", K, level_ids[lv])
        out["kb"] = run_alternating(calls, "kb")
        out["kb"]["docs"] = {str(lv): len(ids) for lv, ids in level_ids.items()}
        out["kb"]["d"] = kb_d
        kb.close()

head = [
    "Labelled search: DeviceIndex.search_batch_labeled (one query, k = 100; the filter on the device) against",
    "DeviceIndex.search_batch_within over the same rows as a prebuilt ascending host list (tools/labels_time.py, MI355X, one",
    "process, the calls alternating call by call).  kb rows: KB.retrieve_at_level against KB.retrieve_within with the level's",
    f"doc ids, an on-disk KB of {kb_docs} docs on three levels (1 %, 9 %, 90 %), d = {kb_d}, f32.",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls, csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the calls.  times in ms.",
    "",
    f"{'dtype':5s} {'call':26s} {'p50':>9s} {'(spread)':>9s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

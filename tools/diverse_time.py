#!/usr/bin/env python3
"""Diverse search (svs_index_search_diverse): host-call time of DeviceIndex.search_batch_diverse for ONE query over a
1M x 1536 corpus built on the device, k = 10, fetch_k in {64, 256, 1024}, beside -- in the same process, alternating
call by call --
  (b) search   DeviceIndex.search_batch at k = fetch_k: the candidate search alone, the floor; (a) - (b) is what the
               re-ranking costs;
  (g) k = 2    the diverse call with k = 2: the search, the whole Gram kernel and ONE pick step; (g) - (b) is the Gram
               kernel's time as a caller sees it, set against 2 c^2 d FLOP;
  (c) host     the route the entry replaces: the search, DeviceIndex.stored_rows per candidate, a numpy Gram matrix and
               the greedy loop in Python (fewer repetitions: it is slow).
Writes a table and one JSON line: per dtype the p50 in ms and the 25th-75th percentile spread of every call.
  usage: diverse_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=30] [out=profiles/diverse_time.txt]"""
import json
import os
import subprocess
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "diverse_time.txt")
K, LAM = 10, 0.5
FETCH = [64, 256, 1024]


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def host_route(idx, q, k, fetch_k, lam):
    s, r = idx.search_batch(q, fetch_k)
    s, r = s[0], r[0]
    R = np.concatenate([idx.stored_rows(int(row), 1) for row in r])
    G = R @ R.T
    picks, red = [0], np.full(len(r), -np.inf, dtype=np.float32)
    free = np.ones(len(r), dtype=bool)
    free[0] = False
    for _ in range(1, min(k, len(r))):
        red = np.maximum(red, G[:, picks[-1]])
        obj = np.where(free, np.float32(lam) * s - np.float32(1 - lam) * red, -np.inf)
        picks.append(int(np.argmax(obj)))
        free[picks[-1]] = False
    return r[picks]


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
    except OSError:
        return "?"


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(15)
out = {"n": n, "d": d, "k": K, "lam": LAM, "csrc_sha16": csrc_sha16(), "commit": commit(), "reps": reps}
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
    q = torch.randn((1, d), device=dev, generator=g)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    calls, slow = {}, {}
    for fk in FETCH:
        calls[f"diverse_k10_fetch_{fk}"] = lambda fk=fk: idx.search_batch_diverse(q, K, fk, LAM)
        calls[f"diverse_k2_fetch_{fk}"] = lambda fk=fk: idx.search_batch_diverse(q, 2, fk, LAM)
        calls[f"search_{fk}"] = lambda fk=fk: idx.search_batch(q, fk)
        slow[f"host_route_fetch_{fk}"] = lambda fk=fk: host_route(idx, q, K, fk, LAM)
    # the two routes' picks, compared (numpy's Gram sums in another order: a near-tie may legitimately differ; reported,
    # not asserted -- tests/test_diverse_gpu.py is the check); the calls are warm afterwards
    agree = {fk: idx.search_batch_diverse(q, K, fk, LAM)[1][0].tolist() == host_route(idx, q, K, fk, LAM).tolist() for fk in (64, 256)}
    print(f"[diverse_time] {dtype} picks equal to the host route's: {agree}", file=sys.stderr, flush=True)
    for fn in calls.values():
        fn()
    times = {name: [] for name in list(calls) + list(slow)}
    for i in range(reps):       # alternating, so that drift hits all alike
        for name, fn in calls.items():
            times[name].append(timed(fn))
        if i < 3:
            for name, fn in slow.items():
                times[name].append(timed(fn))
    res = {}
    for name, v in times.items():
        q25, q50, q75 = np.percentile(v, [25, 50, 75])
        res[name] = {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4), "calls": len(v)}
        lines.append(f"{dtype:5s} {name:26s} {q50:10.4f} {q75 - q25:9.4f} {len(v):6d}")
        print(f"[diverse_time] {dtype} {name}: {res[name]}", file=sys.stderr, flush=True)
    for fk in FETCH:
        c = min(fk, n)
        gram_ms = res[f"diverse_k2_fetch_{fk}"]["p50_ms"] - res[f"search_{fk}"]["p50_ms"]
        mmr_ms = res[f"diverse_k10_fetch_{fk}"]["p50_ms"] - res[f"search_{fk}"]["p50_ms"]
        tf = 2.0 * c * c * d / (gram_ms * 1e-3) / 1e12 if gram_ms > 0 else float("nan")
        res[f"derived_fetch_{fk}"] = {"mmr_ms": round(mmr_ms, 4), "gram_ms": round(gram_ms, 4), "gram_tflops": round(tf, 2)}
        lines.append(f"{dtype:5s} derived fetch_k={fk:5d}: re-ranking {mmr_ms:8.4f} ms, Gram (k = 2 call - search) {gram_ms:8.4f} ms"
                     f" = {tf:6.2f} TFLOP/s of 2 c^2 d")
    out[dtype] = res
    idx.release()
head = [
    "Diverse search: DeviceIndex.search_batch_diverse (one query, k = 10, lambda 0.5) against the candidate search alone and against",
    "the host route it replaces (search + stored_rows per candidate + numpy Gram + Python greedy); tools/diverse_time.py, MI355X, one",
    "process, the calls alternating call by call.",
    f"n = {n}, d = {d}, p50 of the warmed calls, commit {out['commit']} (+ the working tree), csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the calls.  times in ms.",
    "",
    f"{'dtype':5s} {'call':26s} {'p50':>10s} {'(spread)':>9s} {'calls':>6s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

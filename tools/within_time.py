#!/usr/bin/env python3
"""Filtered retrieval (svs_index_search_rows): host-call time of DeviceIndex.search_within / search_batch_within over
m listed rows of a 1M x 1536 corpus, random and contiguous subsets, beside the full search (svs_index_search) on the
same index.  Prints one JSON line: per dtype, full-search and per-subset medians in ms, and the listed-row bytes each
call reads (m x row bytes) for the roofline.  Under `rocprofv3 --kernel-trace --stats` the gather kernel's time per
launch comes from the trace (tools/ has no counters in this script).
  usage: within_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=30]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from svs_amd import DeviceIndex
from svs_amd.buildinfo import csrc_sha16

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 1536
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
k = 100


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
    return round(float(np.median(t)) * 1e3, 4)


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(11)
rng = np.random.default_rng(11)
Q = torch.randn((16, d), device=dev, generator=g)
Q = (Q / Q.norm(dim=1, keepdim=True)).cpu().numpy()
out = {"n": n, "d": d, "k": k, "csrc_sha16": csrc_sha16(), "reps": reps}
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        v = torch.randn((rows, d), device=dev, generator=g)
        v /= v.norm(dim=1, keepdim=True)
        idx.append_device(v.contiguous().data_ptr(), rows)
        del v
    torch.cuda.synchronize()
    row_bytes = idx.ld * {"f32": 4, "f16": 2, "fp8": 1}[dtype]
    res = {"row_bytes": row_bytes,
           "full_nq1_ms": median_ms(lambda: idx.search(Q[0], k), reps),
           "full_nq16_ms": median_ms(lambda: idx.search_batch(Q, k), reps)}
    for kind in ("random", "contiguous"):
        for m in (1_000, 10_000, 100_000, n):
            if kind == "random":
                rows = np.sort(rng.choice(n, m, replace=False)) if m < n else np.arange(n)
            else:
                r0 = int(rng.integers(0, n - m + 1))
                rows = np.arange(r0, r0 + m)
            res[f"{kind}_{m}"] = {
                "listed_bytes": m * row_bytes,
                "nq1_ms": median_ms(lambda: idx.search_within(Q[0], k, rows), reps),
                "nq16_ms": median_ms(lambda: idx.search_batch_within(Q, k, rows), max(reps // 3, 5)),
            }
            print(f"[within_time] {dtype} {kind} m={m}: {res[f'{kind}_{m}']}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
print(json.dumps(out), flush=True)

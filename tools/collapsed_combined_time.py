#!/usr/bin/env python3
"""Group-combined search (svs_index_search_collapsed_combined): host-call time of
DeviceIndex.search_batch_collapsed_combined for ONE combined query of m = 2, 4, 8 vectors, k = 100, op = "min",
zero = "single", over a 1M x 1536 corpus built on the device, for two group layouts of column 1
  adj8     runs of 8 adjacent rows: n / 8 groups (125,000 at 1M rows)
  own      every row its own value: n groups (the table at its fullest)
beside -- in the same process and session, alternating call by call (an untimed call behind every (c): the GPU idles
while numpy works) --
  (a) combined      DeviceIndex.search_batch_combined at the same m: the FLOOR, it reads the same corpus bytes once and
                    ranks rows, not groups,
  (b) collapsed x m DeviceIndex.search_batch_collapsed with the m vectors as m queries: m corpus passes and m group
                    stages -- and not the answer (each vector's groups ranked on their own),
  (c) numpy         m x DeviceIndex.scores + the grouping in numpy over a host copy of the column: what a caller can do
                    without the entry, exactly.
(c)'s answer is checked to equal the entry's.  Then, with svs_index_set_timing on, the split of the call between its
stages from the HIP events around them (svs_internal_collapsed_combined_kernel_ms): the score pass, the reduce kernel,
the mark kernel, the two fills, the top-k stage.  Last, the multi-score kernel against the combine_* kernel of the same
shape and m, each from the events around it in its test hook (svs_internal_score_pass_ms; fused route forced).
Writes a table and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call, and the ratios.
  usage: collapsed_combined_time.py [n=1000000] [d=1536] [dtypes=f32,f16,fp8] [reps=30] [out=profiles/collapsed_combined_time.txt]"""
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
dtypes = (sys.argv[3] if len(sys.argv) > 3 else "f32,f16,fp8").split(",")
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 30
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "collapsed_combined_time.txt")
K = 100
COLUMN = 1
OP = "min"
MS = [2, 4, 8]
LAYOUTS = ["adj8", "own"]
STAGES = ["scores", "reduce", "mark", "clear", "select"]
lib = _native.load()


def column_of(layout):
    r = np.arange(n, dtype=np.int64)
    return (r // 8 + 1 if layout == "adj8" else r + 1).astype(np.uint32)


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def entry(idx, v):
    s, r, val, counts, groups = idx.search_batch_collapsed_combined(v[None], K, COLUMN, OP, None, "single")
    c = int(counts[0])
    return s[0, :c], r[0, :c], val[0, :c], int(groups[0])


def numpy_groups(idx, v, col, starts):
    """The definition for "min", no weights, no value 0, no dead row, finite scores; col is sorted (both layouts are)."""
    s = np.stack([idx.scores(x) for x in v])
    best = np.maximum.reduceat(s, starts, axis=1).min(axis=0)                 # c(G) = min_j max_r s_j[r]
    c_row = s.min(axis=0)
    order = np.lexsort((np.arange(n), c_row, col))                             # by value, then row-level score, then row
    rep = order[np.append(starts[1:], n) - 1]
    rank = np.lexsort((rep, best))[::-1][:K]
    return best[rank], rep[rank], col[rep[rank]], len(starts)


def stats(t):
    q25, q50, q75 = np.percentile(t, [25, 50, 75])
    return {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}


def hook_ms(idx, v, multi):
    """Median of the events around the fused score pass of one hook call (route 1), ms."""
    m = v.shape[0]
    out = np.empty(m * n if multi else n, dtype=np.float32)
    ms = C.c_double(0.0)
    got = []
    for _ in range(reps):
        if multi:
            _native.check(lib.svs_internal_multi_scores(idx._handle(), v.ctypes.data, m, d, 1, out.ctypes.data, out.size))
        else:
            _native.check(lib.svs_internal_combined_scores(idx._handle(), v.ctypes.data, m, d, None, _native.COMBINE_MIN, 1, out.ctypes.data, out.size))
        _native.check(lib.svs_internal_score_pass_ms(C.byref(ms)))
        got.append(ms.value)
    return round(float(np.median(got)), 4)


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(17)
out = {"n": n, "d": d, "k": K, "op": OP, "csrc_sha16": csrc_sha16(), "reps": reps}
lines, split_lines, kernel_lines = [], [], []
for dtype in dtypes:
    idx = DeviceIndex.empty(d, device=0, dtype=dtype, reserve=n)
    for r0 in range(0, n, 250_000):
        rows = min(250_000, n - r0)
        x = torch.randn((rows, d), device=dev, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        idx.append_device(x.contiguous().data_ptr(), rows)
        del x
    torch.cuda.synchronize()
    vec = torch.randn((max(MS), d), device=dev, generator=g)
    vec = np.ascontiguousarray((vec / vec.norm(dim=1, keepdim=True)).cpu().numpy())
    res = {}
    for layout in LAYOUTS:
        col = column_of(layout)
        starts = np.nonzero(np.append(True, col[1:] != col[:-1]))[0]
        idx.set_column(COLUMN, col)
        for m in MS:
            v = np.ascontiguousarray(vec[:m])
            # (c) keeps the host busy for a long time while the GPU idles, and the call behind such a pause is slower
            # whatever it is: (c) goes first and an untimed call follows it
            calls = {"numpy": lambda: numpy_groups(idx, v, col, starts),
                     "(untimed)": lambda: idx.search_batch_combined(v[None], K, OP),
                     "entry": lambda: entry(idx, v),
                     "combined": lambda: idx.search_batch_combined(v[None], K, OP),
                     "collapsed_x_m": lambda: idx.search_batch_collapsed(v, K, COLUMN, "single")}
            es, er, ev, eg = numpy_groups(idx, v, col, starts)
            s, r, val, groups = entry(idx, v)
            assert groups == eg and r.tolist() == er.tolist() and val.tolist() == ev.tolist() and s.tolist() == es.tolist(), (dtype, layout, m)
            c_reps = max(3, reps // 10)                                  # (c) sorts n rows on the host: a few runs are enough
            times = {name: [] for name in calls}
            for i in range(reps):       # alternating, so that drift hits all alike
                for name, fn in calls.items():
                    if name == "numpy" and i >= c_reps:
                        continue
                    times[name].append(timed(fn))
            r_ = {name: stats(t) for name, t in times.items() if name != "(untimed)"}
            # the split, from the events around the stages (their own calls: the events cost a little)
            idx.set_timing(1)
            ms = (C.c_double * 5)()
            parts = [[] for _ in STAGES]
            for _ in range(reps):
                entry(idx, v)
                _native.check(lib.svs_internal_collapsed_combined_kernel_ms(ms))
                for i in range(5):
                    parts[i].append(ms[i])
            split = {st: round(float(np.median(p)), 4) for st, p in zip(STAGES, parts)}
            kern = None
            if layout == LAYOUTS[0]:    # (the score kernels do not read the column)
                kern = {"multi_score_ms": hook_ms(idx, v, True), "combine_ms": hook_ms(idx, v, False)}
                kern["ratio"] = round(kern["multi_score_ms"] / kern["combine_ms"], 3)
                kernel_lines.append(f"{dtype:5s} {m:2d} {kern['multi_score_ms']:12.4f} {kern['combine_ms']:10.4f} {kern['ratio']:7.3f}")
            idx.set_timing(0)
            a, fl, cm, np_ = (r_[k]["p50_ms"] for k in ("entry", "combined", "collapsed_x_m", "numpy"))
            r_.update(groups=int(groups), split_ms=split, ratio_to_combined=round(a / fl, 3), collapsed_x_m_over_entry=round(cm / a, 3),
                      numpy_over_entry=round(np_ / a, 2), kernels=kern)
            res[f"{layout}/m{m}"] = r_
            lines.append(f"{dtype:5s} {layout:5s} {m:2d} {int(groups):9d} {a:9.4f} {r_['entry']['spread_ms']:8.4f} {fl:9.4f} {cm:10.4f} {np_:10.3f} "
                         f"{a / fl:7.3f} {cm / a:7.3f} {np_ / a:8.2f}")
            split_lines.append(f"{dtype:5s} {layout:5s} {m:2d} " + " ".join(f"{split[st]:8.4f}" for st in STAGES) + f" {sum(split.values()):8.4f}")
            print(f"[collapsed_combined_time] {lines[-1]} | {split_lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Group-combined search: DeviceIndex.search_batch_collapsed_combined (one combined query of m vectors, k = 100, op = min, column 1, zero = single)",
    "against (a) search_batch_combined at the same m -- the floor: the same corpus bytes, rows ranked instead of groups --, (b) search_batch_collapsed",
    "with the m vectors as m queries (m corpus passes; not the answer) and (c) m x DeviceIndex.scores + the grouping in numpy (exact; checked equal)",
    "(tools/collapsed_combined_time.py, MI355X, one process, the calls alternating call by call, one untimed call behind every (c)).",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls ((c): of {max(3, reps // 10)}), csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the entry's calls.  times in ms.  layout adj8: runs of 8 adjacent rows; own: every row its own value.",
    "/(a): the entry over (a); (b)/, (c)/: (b) and (c) over the entry.",
    "",
    f"{'dtype':5s} {'layout':5s} {'m':>2s} {'groups':>9s} {'entry':>9s} {'(spread)':>8s} {'(a) comb.':>9s} {'(b) coll.xm':>10s} {'(c) numpy':>10s} "
    f"{'/(a)':>7s} {'(b)/':>7s} {'(c)/':>8s}",
]
mid = ["", "The stages of the call's one query, from the HIP events around them (svs_index_set_timing on; median of the same number of calls, ms;",
       "scores = the fused multi-score kernel, clear = the fills of the table and of the per-vector keys):",
       f"{'dtype':5s} {'layout':5s} {'m':>2s} " + " ".join(f"{st:>8s}" for st in STAGES) + f" {'sum':>8s}"]
tail = ["", "The fused multi-score kernel (m scores stored per row) against the fused combine kernel of the same shape and m (one score stored per row),",
        "each from the events around it in its test hook, fused route forced (median, ms).  No wave-level fold of the m keys was tried in the reduce kernel.",
        f"{'dtype':5s} {'m':>2s} {'multi_score':>12s} {'combine':>10s} {'ratio':>7s}"]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines + mid + split_lines + tail + kernel_lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

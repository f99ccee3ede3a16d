#!/usr/bin/env python3
"""Per-label breakdown (svs_index_search_by_label): host-call time of DeviceIndex.search_batch_by_label for ONE query
over a 1M x 1536 corpus built on the device, for sets of 1, 16 and 1,024 labels, two label layouts (the set's labels
spread uniformly over the rows; ONE label of the set holding every row) and three cut-offs (admitting about 100 rows,
1 % of the rows, every row), beside -- in the same process and session, alternating call by call (an untimed call behind every (ii): the GPU idles while numpy works) --
  (i)  above   DeviceIndex.search_batch_above, count only, at the same cut-off: the floor (one score pass plus one
               filter over the same score vector), and
  (ii) numpy   DeviceIndex.scores + a numpy group-by over a host copy of the labels: what a caller can do without the
               entry.
Every configuration is timed under both cross-workgroup routes of the reduce kernel (svs_internal_tune(7, v): integer
atomics on a table in HBM; one partial table per workgroup) and the three answers are checked to agree.  Writes a table
and one JSON line: the p50 in ms and the 25th-75th percentile spread of every call, the ratio to (i) and to (ii).
  usage: by_label_time.py [n=1000000] [d=1536] [dtypes=f32,f16] [reps=40] [out=profiles/by_label_time.txt]"""
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
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "by_label_time.txt")
SETS = [1, 16, 1024]
LAYOUTS = ["uniform", "one"]
CUTS = ["100", "1pct", "all"]
lib = _native.load()


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


def numpy_group_by(idx, q, lab, label_set, cut):
    s = idx.scores(q)
    rows = np.nonzero(s >= cut)[0]
    rows = rows[np.isin(lab[rows], label_set)]
    order = np.lexsort((rows, s[rows], lab[rows]))
    rows = rows[order]
    found, first, totals = np.unique(lab[rows], return_index=True, return_counts=True)
    best = rows[first + totals - 1]
    rank = np.lexsort((best, s[best]))[::-1]
    return found[rank], s[best[rank]], best[rank], totals[rank]


def by_label(idx, q, label_set, cut, cross):
    lib.svs_internal_tune(7, cross)
    try:
        return idx.search_batch_by_label(q, label_set, [cut])[0]
    finally:
        lib.svs_internal_tune(7, 0)


def stats(v):
    q25, q50, q75 = np.percentile(v, [25, 50, 75])
    return {"p50_ms": round(float(q50), 4), "spread_ms": round(float(q75 - q25), 4)}


dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(15)
out = {"n": n, "d": d, "csrc_sha16": csrc_sha16(), "reps": reps}
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
    ranked = np.sort(idx.scores(q[0]))[::-1]
    cuts = {"100": ranked[99], "1pct": ranked[n // 100 - 1], "all": np.float32(-np.inf)}
    res = {}
    for nset in SETS:
        label_set = (np.arange(nset, dtype=np.uint32) * 3 + 5)
        for layout in LAYOUTS:
            lab = label_set[np.arange(n) % nset] if layout == "uniform" else np.full(n, label_set[nset // 2], dtype=np.uint32)
            idx.set_labels(lab)
            for cname in CUTS:
                cut = cuts[cname]
                # (ii) keeps the host busy for up to 150 ms while the GPU idles, and the call behind such a pause is
                # ~0.15 ms slower whatever it is: (ii) goes first and an untimed call follows it
                calls = {"numpy_group_by": lambda: numpy_group_by(idx, q[0], lab, label_set, cut),
                         "(untimed)": lambda: idx.search_batch_above(q, [cut], 0),
                         "by_label": lambda: by_label(idx, q, label_set, cut, 0),
                         "by_label_partials": lambda: by_label(idx, q, label_set, cut, 1),
                         "above_count": lambda: idx.search_batch_above(q, [cut], 0)}
                # the three agree (and the calls are warm afterwards)
                el, es, er, et = numpy_group_by(idx, q[0], lab, label_set, cut)
                for cross in (0, 1):
                    l, s, r, t, groups = by_label(idx, q, label_set, cut, cross)
                    assert groups == len(el) and l.tolist() == el.tolist() and r.tolist() == er.tolist(), (dtype, nset, layout, cname, cross)
                    assert s.tolist() == es.tolist() and t.tolist() == et.tolist(), (dtype, nset, layout, cname, cross)
                assert int(et.sum()) == idx.search_batch_above(q, [cut], 0)[0][2]
                times = {name: [] for name in calls}
                for _ in range(reps):       # alternating, so that drift hits all alike
                    for name, fn in calls.items():
                        times[name].append(timed(fn))
                r_ = {name: stats(v) for name, v in times.items() if name != "(untimed)"}
                a, p, fl, np_ = (r_[k]["p50_ms"] for k in ("by_label", "by_label_partials", "above_count", "numpy_group_by"))
                r_["ratio_to_above"] = round(a / fl, 3)
                r_["ratio_partials_to_above"] = round(p / fl, 3)
                r_["numpy_over_by_label"] = round(np_ / a, 2)
                r_["rows_admitted"] = int(et.sum())
                res[f"{nset}_{layout}_{cname}"] = r_
                lines.append(f"{dtype:5s} {nset:5d} {layout:8s} {cname:5s} {int(et.sum()):9d} {a:9.4f} {r_['by_label']['spread_ms']:8.4f} {p:9.4f} "
                             f"{fl:9.4f} {np_:10.4f} {a / fl:7.3f} {p / fl:7.3f} {np_ / a:8.2f}")
                print(f"[by_label_time] {lines[-1]}", file=sys.stderr, flush=True)
    out[dtype] = res
    idx.release()
head = [
    "Per-label breakdown: DeviceIndex.search_batch_by_label (one query, every label of the set asked for) against (i) search_batch_above,",
    "count only, at the same cut-off and (ii) DeviceIndex.scores + a numpy group-by over a host copy of the labels (tools/by_label_time.py,",
    "MI355X, one process, the calls alternating call by call, one untimed call behind every (ii)).  atomic / partials: the two cross-workgroup routes of the reduce kernel",
    "(svs_internal_tune(7, 0 / 1)); atomic is the default.",
    f"n = {n}, d = {d}, p50 of {reps} warmed calls, csrc_sha16 {out['csrc_sha16']}",
    "spread = 75th - 25th percentile of the atomic route's calls.  times in ms.  layout uniform: the set's labels dealt over the rows;",
    "one: one label of the set holds every row.  cut 100 / 1pct / all: the cut-off admits about 100 rows, 1 % of the rows, every row (-inf).",
    "",
    f"{'dtype':5s} {'set':>5s} {'layout':8s} {'cut':5s} {'admitted':>9s} {'atomic':>9s} {'(spread)':>8s} {'partials':>9s} {'(i) above':>9s} {'(ii) numpy':>10s} "
    f"{'a/(i)':>7s} {'p/(i)':>7s} {'(ii)/a':>8s}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n\nraw: " + json.dumps(out) + "\n")
print(json.dumps(out), flush=True)

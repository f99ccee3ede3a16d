"""GPU: bench.py's plain run and `--dump-outputs`.  A plain run times the steps and prints the headline only (the
secondary figures are `--full`'s); the dumped arrays are the answer of the LAST timed step, the same as one search of
that step's query on an index over the same seeded corpus."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_step(gpu, tmp_path):
    n, d, k, steps, warmup, seed = 200_000, 1536, 100, 7, 3, 1234
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", str(n), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["batched"] is None and line["concurrent"] is None and line["configs"] == [] and line["p50_latency_ms"] is None
    assert "cpu_baseline" not in line and "parity_spot_check" not in line

    scores, rows = np.load(out / "scores.npy"), np.load(out / "rows.npy")
    assert scores.dtype == np.float32 and rows.dtype == np.float64 and scores.shape == rows.shape == (k,)

    import torch
    import bench
    from svs_amd import DeviceIndex
    dev = torch.device("cuda", 0)
    m = bench.gen_rows(torch, dev, seed, 0, n, d)
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 77)
    q = torch.randn((warmup + steps, d), device=dev, dtype=torch.float32, generator=g)
    q /= q.norm(dim=1, keepdim=True)
    torch.cuda.synchronize()
    idx = DeviceIndex.from_device_pointer(m.data_ptr(), n, d, device=0)
    exp = idx.search(q[warmup + steps - 1].cpu().numpy(), k)
    idx.release()
    assert [int(x) for x in rows] == [r_ for _, r_ in exp]
    assert np.max(np.abs(scores - np.array([s for s, _ in exp], dtype=np.float32))) <= 1e-6

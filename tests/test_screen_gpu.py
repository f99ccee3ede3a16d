"""GPU: the screened single-query search of an f32 index (svs_amd/csrc/screen.h) returns what the unscreened search
returns -- rows, order and score BITS -- on every case below, and the kernels it is made of really ran.

A case searches one index twice: with svs_index_set_variant(11) (never screened: the launches of the f32 path) and
with screening on (variant 0 on corpora of at least screen_min_rows() rows, variant 12 -- "screen whatever n" -- on the
small ones).  svs_internal_last_launches says which score kernels were enqueued, svs_internal_screen_stats which branch
(candidate list / exact whole-corpus fallback) the re-score kernel took.

The bound E >= |approximate - exact| ("Screened search") is checked against the real kernels: an f16 index
over the same rows returns exactly the screen kernel's scores.
"""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from single_kernel_table import _f16_oneshot
from svs_amd import DeviceIndex, _native

OFF, FORCE = 11, 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gaussian(n, d, seed, unit=True):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, d), dtype=np.float32)
    if unit:
        m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


def uniform_recipe(n, d, seed):
    """The reference notebook's corpus: uniform [0, 1) rows, normalised (top scores ~0.77, adjacent gaps ~3e-7)."""
    rng = np.random.default_rng(seed)
    m = rng.random((n, d), dtype=np.float32)
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    return m


def unit(v):
    v = np.asarray(v, dtype=np.float32)
    return v / np.linalg.norm(v)


def is_screen(name):
    return name.startswith("gemv_f16_oneshot_kernel<") or name.startswith("rescore_f32_kernel<")


def check(idx, q, k, expect, on=FORCE, label="", names=None):
    """expect: 'list' (answered from the candidate list), 'fallback' (exact whole-corpus re-score), 'any' (screened,
    either branch), 'off' (the screened variant must NOT screen this call).  names: the exact (screen pass, re-score)
    kernels a screened call must have launched."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    idx.set_variant(OFF)
    s0, r0 = idx.search_batch(q[None, :], k)
    l0 = _native.last_launches()
    assert not [x for x in l0 if is_screen(x[0])], (label, l0)
    idx.set_variant(on)
    before = idx.screen_stats()
    s1, r1 = idx.search_batch(q[None, :], k)
    l1 = _native.last_launches()
    after = idx.screen_stats()
    idx.set_variant(0)
    assert np.array_equal(r0, r1), (label, np.flatnonzero(r0[0] != r1[0])[:8])
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (label, np.flatnonzero(s0.view(np.uint32)[0] != s1.view(np.uint32)[0])[:8])
    ds, df = after["screened"] - before["screened"], after["fallback"] - before["fallback"]
    print(f"{label}: n={idx.n} d={idx.d} k={k} screened+{ds} fallback+{df} E={after['E']:.3e} n_cand={after['n_cand']}")
    if expect == "off":
        assert not [x for x in l1 if is_screen(x[0])], (label, l1)
        assert (ds, df) == (0, 0), (label, ds, df)
        return s1, r1
    assert len(l1) == 2 and l1[0][0].startswith("gemv_f16_oneshot_kernel<") and l1[0][1:] == (idx.n, 1), (label, l1)
    assert l1[1][0].startswith("rescore_f32_kernel<") and l1[1][1:] == (idx.n, 1), (label, l1)
    if names is not None:
        assert (l1[0][0], l1[1][0]) == tuple(names), (label, l1, names)
    assert ds + df == 1, (label, ds, df)
    if expect == "list":
        assert ds == 1, (label, after)
    elif expect == "fallback":
        assert df == 1, (label, after)
    return s1, r1


# ---- the two corpora that need size: default variant, n >= screen_min_rows() ----------------------------------------
@pytest.mark.parametrize("recipe", ["gaussian", "uniform"])
@pytest.mark.gpu
def test_large_corpus_d1536(gpu, recipe):
    n, d = 200_000, 1536
    m = gaussian(n, d, 1) if recipe == "gaussian" else uniform_recipe(n, d, 2)
    idx = DeviceIndex(m, device=0)
    assert idx.screen_stats()["shadow"] == 1
    assert idx.hbm_bytes == n * d * 4 + n * d * 2
    rng = np.random.default_rng(3)
    for j in range(4):
        q = unit(rng.standard_normal(d)) if recipe == "gaussian" else unit(rng.random(d))
        check(idx, q, 100, "list", on=0, label=f"{recipe} q{j}")
    check(idx, unit(m[77] + 0.1 * rng.standard_normal(d).astype(np.float32)), 1, "list", on=0, label=f"{recipe} k=1")
    check(idx, unit(rng.standard_normal(d)) if recipe == "gaussian" else unit(rng.random(d)), 2048, "list", on=0, label=f"{recipe} k=2048")
    check(idx, unit(rng.standard_normal(d)) if recipe == "gaussian" else unit(rng.random(d)), 2049, "off", on=0, label=f"{recipe} k=2049")
    idx.release()


def screen_kernels(d):
    """The shadow pass and the re-score of an f32 index of d = ld floats: gemv_f16_oneshot_kernel<d / 512, R, WPB> as
    an f16 index of that row length launches it, rescore_f32_kernel<d / 256, U> with U = 4, 2, 1 (rescore_u)."""
    nstep = d // 256
    return _f16_oneshot(d // 512), f"rescore_f32_kernel<{nstep}, {4 if nstep <= 4 else 2 if nstep <= 8 else 1}>"


@pytest.mark.parametrize("d", [512, 1024, 1536, 2048, 2560, 3072, 3584, 4096])
@pytest.mark.gpu
def test_other_row_lengths(gpu, d):
    """Every row length that has a shadow: each of the eight rescore_f32_kernel instantiations and of the eight shadow
    passes, by name."""
    n = 12_000
    m = gaussian(n, d, 10 + d)
    idx = DeviceIndex(m, device=0)
    assert idx.ld == d
    rng = np.random.default_rng(d)
    for k in (1, 100, 2048):
        check(idx, unit(rng.standard_normal(d)), k, "list", label=f"d={d} k={k}", names=screen_kernels(d))
    check(idx, unit(rng.standard_normal(d)), 2049, "off", label=f"d={d} k=2049")
    idx.release()


@pytest.mark.gpu
def test_small_corpus_is_not_screened_by_default(gpu):
    m = gaussian(6000, 512, 5)
    idx = DeviceIndex(m, device=0)
    check(idx, unit(np.random.default_rng(6).standard_normal(512)), 10, "off", on=0, label="below the minimum row count")
    idx.release()


@pytest.mark.gpu
def test_unsupported_row_length_has_no_shadow(gpu):
    m = gaussian(6000, 384, 5)
    idx = DeviceIndex(m, device=0)
    assert idx.screen_stats()["shadow"] == 0 and idx.hbm_bytes == 6000 * idx.ld * 4
    check(idx, unit(np.random.default_rng(6).standard_normal(384)), 10, "off", label="d=384")
    idx.release()


@pytest.mark.gpu
def test_duplicate_rows_across_the_kth_place(gpu):
    n, d, k = 8000, 1536, 100
    m = gaussian(n, d, 20)
    q = unit(np.random.default_rng(21).standard_normal(d))
    order = np.argsort(-(m.astype(np.float64) @ q.astype(np.float64)))
    kth = m[order[k - 21]].copy()
    dup = np.random.default_rng(22).choice(order[2000:], 40, replace=False)
    m[dup] = kth                      # 41 bit-identical rows straddle the k-th place: the tie is cut by row, descending
    idx = DeviceIndex(m, device=0)
    s, r = check(idx, q, k, "list", label="duplicates")
    tied = np.flatnonzero(s[0].view(np.uint32) == s[0].view(np.uint32)[k - 1])
    assert len(tied) >= 2 and np.all(np.diff(r[0][tied]) < 0)
    idx.release()


@pytest.mark.gpu
def test_mass_near_duplicates_overflow_to_the_fallback(gpu):
    n, d = 50_000, 512
    rng = np.random.default_rng(30)
    base = unit(rng.standard_normal(d))
    m = base[None, :] + 1e-6 * rng.standard_normal((n, d), dtype=np.float32)   # every score within E of every other
    idx = DeviceIndex(m.astype(np.float32), device=0)
    check(idx, base, 100, "fallback", label="50,000 near copies")
    idx.release()


@pytest.mark.gpu
def test_query_edge_cases(gpu):
    n, d = 8000, 1536
    m = uniform_recipe(n, d, 40)
    idx = DeviceIndex(m, device=0)
    rng = np.random.default_rng(41)
    q = unit(rng.random(d))
    check(idx, -q, 100, "fallback", label="all scores negative")
    check(idx, q * np.float32(1e3), 100, "list", label="query x 1e3")
    check(idx, q * np.float32(1e-3), 100, "list", label="query x 1e-3")
    check(idx, np.zeros(d, np.float32), 100, "fallback", label="zero query")
    qn = q.copy()
    qn[17] = np.nan
    check(idx, qn, 100, "fallback", label="NaN in the query")
    check(idx, q * np.float32(1e30), 100, "fallback", label="query that overflows half")
    idx.release()


@pytest.mark.gpu
def test_row_norms_over_four_decades(gpu):
    n, d = 10_000, 1536
    rng = np.random.default_rng(50)
    m = gaussian(n, d, 51) * (10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    idx = DeviceIndex(m, device=0)
    st = idx.screen_stats()
    assert st["C"] >= float(np.linalg.norm(m.astype(np.float64), axis=1).max())
    for j in range(3):
        check(idx, unit(rng.standard_normal(d)), 100, "any", label=f"norm spread q{j}")
    idx.release()


@pytest.mark.gpu
def test_half_overflow_never_screens(gpu):
    n, d = 8000, 1536
    m = gaussian(n, d, 60)
    m[1234, 5] = 1e5
    idx = DeviceIndex(m, device=0)
    assert idx.screen_stats()["shadow"] == 2
    check(idx, unit(np.random.default_rng(61).standard_normal(d)), 100, "off", label="element 1e5")
    idx.append(gaussian(100, d, 62))          # invalid for good
    check(idx, unit(np.random.default_rng(63).standard_normal(d)), 100, "off", label="element 1e5, after an append")
    idx.release()


@pytest.mark.gpu
def test_tombstones_among_the_winners(gpu):
    n, d = 9000, 1536
    m = gaussian(n, d, 70)
    q = unit(np.random.default_rng(71).standard_normal(d))
    idx = DeviceIndex(m, device=0)
    s, r = check(idx, q, 100, "list", label="before masking")
    dead = r[0][[0, 3, 50, 99]]
    idx.mask_rows(dead)
    s2, r2 = check(idx, q, 100, "list", label="after masking")
    assert not set(dead.tolist()) & set(r2[0].tolist())
    check(idx, unit(m[5]), 100, "any", label="masked, other query")
    idx.release()


@pytest.mark.gpu
def test_masked_rows_in_the_fallback(gpu):
    n, d = 8000, 1536
    m = uniform_recipe(n, d, 72)
    q = -unit(np.random.default_rng(73).random(d))
    idx = DeviceIndex(m, device=0)
    s, r = check(idx, q, 50, "fallback", label="fallback before masking")
    idx.mask_rows(r[0][:5])
    s2, r2 = check(idx, q, 50, "fallback", label="fallback after masking")
    assert not set(r[0][:5].tolist()) & set(r2[0].tolist())
    idx.release()


@pytest.mark.gpu
def test_rows_appended_after_creation(gpu):
    import torch
    d = 1536
    rng = np.random.default_rng(80)
    q = unit(rng.standard_normal(d))
    near = lambda cnt, seed: ((q[None, :] + 0.05 * np.random.default_rng(seed).standard_normal((cnt, d)))).astype(np.float32)
    idx = DeviceIndex(gaussian(6000, d, 81), device=0)
    c0 = idx.screen_stats()["C"]
    idx.append(near(1500, 82))                                    # from the host
    t = torch.from_numpy(near(1500, 83)).cuda()
    idx.append_device(t.data_ptr(), 1500)                         # from device memory
    blk = idx.staging_acquire()
    blk[:1200] = near(1200, 84)
    idx.staging_commit(1200)                                      # through the staging blocks
    s, r = check(idx, q, 100, "list", label="after three appends")
    idx.staging_finish()
    assert idx.n == 10_200 and r[0].min() >= 6000                 # the winners are appended rows
    st = idx.screen_stats()
    assert st["shadow"] == 1 and st["C"] > c0 and st["C"] >= 2.0  # the statistics followed
    assert idx.hbm_bytes >= idx.n * d * 6
    idx.release()


@pytest.mark.gpu
def test_index_built_from_empty_by_staging(gpu):
    d = 512
    idx = DeviceIndex(np.zeros((0, d), np.float32), device=0)
    idx.reserve(9000)
    m = gaussian(9000, d, 85)
    for r0 in range(0, 9000, 3000):
        blk = idx.staging_acquire()
        blk[:3000] = m[r0:r0 + 3000]
        idx.staging_commit(3000)
    check(idx, unit(np.random.default_rng(86).standard_normal(d)), 100, "list", label="staged from empty")
    idx.staging_finish()
    idx.release()


@pytest.mark.gpu
def test_row_offset(gpu):
    m = gaussian(7000, 1536, 90)
    idx = DeviceIndex(m, device=0, row_offset=123_456)
    s, r = check(idx, unit(np.random.default_rng(91).standard_normal(1536)), 100, "list", label="row_offset")
    assert r.min() >= 123_456
    idx.release()


@pytest.mark.gpu
def test_device_entry_sixteen_queries_back_to_back(gpu):
    import torch
    n, d, k = 9000, 1536, 100
    idx = DeviceIndex(gaussian(n, d, 100), device=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(101)
    qs = torch.randn((16, d), device="cuda", generator=g)
    qs /= qs.norm(dim=1, keepdim=True)
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for variant in (OFF, FORCE):
        idx.set_variant(variant)
        out_s = torch.full((16, k), -1.0, device="cuda")
        out_r = torch.full((16, k), -1, device="cuda", dtype=torch.int64)
        before = idx.screen_stats()
        for j in range(16):                                        # no synchronisation in between
            idx.search_device(qs[j].data_ptr(), 1, d, k, out_s[j].data_ptr(), out_r[j].data_ptr(), stream=st)
        torch.cuda.synchronize()
        after = idx.screen_stats()
        res[variant] = (out_s.cpu().numpy(), out_r.cpu().numpy(), after["screened"] - before["screened"])
    idx.set_variant(0)
    assert res[OFF][2] == 0 and res[FORCE][2] == 16
    assert np.array_equal(res[OFF][1], res[FORCE][1])
    assert np.array_equal(res[OFF][0].view(np.uint32), res[FORCE][0].view(np.uint32))
    idx.release()


@pytest.mark.gpu
def test_two_threads_on_one_handle(gpu):
    n, d, k = 9000, 1536, 100
    idx = DeviceIndex(gaussian(n, d, 110), device=0)
    qs = gaussian(24, d, 111)
    idx.set_variant(OFF)
    want = [idx.search_batch(q[None, :], k) for q in qs]
    idx.set_variant(FORCE)
    got, errs = {}, []

    def work(t):
        try:
            for j in range(t, len(qs), 2):
                got[j] = idx.search_batch(qs[j][None, :], k)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    before = idx.screen_stats()
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    after = idx.screen_stats()
    idx.set_variant(0)
    assert not errs, errs
    assert after["screened"] - before["screened"] == len(qs)
    for j, (s, r) in enumerate(want):
        assert np.array_equal(r, got[j][1]) and np.array_equal(s.view(np.uint32), got[j][0].view(np.uint32)), j
    idx.release()


@pytest.mark.parametrize("recipe,d", [("gaussian", 1536), ("uniform", 1536), ("gaussian", 512), ("spread", 4096)])
@pytest.mark.gpu
def test_bound_holds_on_the_real_kernels(gpu, recipe, d):
    """max |a - s| <= E: a from the f16 single-query kernel (an f16 index over the same rows scores with exactly the
    screen kernel), s from the f32 kernel, E as the filter kernel computed it for that query."""
    n = 20_000
    rng = np.random.default_rng(120 + d)
    if recipe == "uniform":
        m = uniform_recipe(n, d, 121)
    else:
        m = gaussian(n, d, 122)
        if recipe == "spread":
            m = m * (10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
    f32 = DeviceIndex(m, device=0)
    f16 = DeviceIndex(m, device=0, dtype="f16")
    f32.set_variant(FORCE)
    for j in range(8):
        q = unit(rng.random(d)) if recipe == "uniform" else unit(rng.standard_normal(d))
        if j >= 6:
            q = q * np.float32(37.0 if j == 6 else 1e-3)
        f32.search_batch(q[None, :], 10)
        E = f32.screen_stats()["E"]
        a, s = f16.scores(q), f32.scores(q)
        err = float(np.abs(a.astype(np.float64) - s.astype(np.float64)).max())
        print(f"bound {recipe} d={d} q{j}: max|a-s| = {err:.3e}  E = {E:.3e}  ratio {E / max(err, 1e-300):.1f}")
        assert np.isfinite(E) and err <= E, (recipe, d, j, err, E)
    f32.release()
    f16.release()


@pytest.mark.gpu
def test_fallbacks_that_dominate_pause_screening_until_the_next_ingest(gpu):
    n, d = 8000, 512
    m = uniform_recipe(n, d, 130)
    idx = DeviceIndex(m, device=0)
    idx.set_variant(FORCE)
    q = -unit(np.random.default_rng(131).random(d))
    for _ in range(40):
        idx.search_batch(q[None, :], 10)
    st = idx.screen_stats()
    assert st["paused"] and 32 <= st["fallback"] < 40, st
    idx.append(uniform_recipe(10, d, 132))
    idx.search_batch(-q[None, :], 10)
    st2 = idx.screen_stats()
    assert not st2["paused"] and st2["screened"] == st["screened"] + 1, st2
    idx.release()


# ---- memory and robustness -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hbm_bytes_and_set_screen_at_full_size(gpu):
    import torch
    n, d, k = 1_000_000, 1536, 100
    g = torch.Generator(device="cuda")
    g.manual_seed(140)
    rows = torch.randn((n, d), device="cuda", generator=g)
    rows /= rows.norm(dim=1, keepdim=True)
    idx = DeviceIndex.from_device_pointer(rows.data_ptr(), n, d, device=0)
    del rows
    torch.cuda.empty_cache()
    assert idx.hbm_bytes == n * d * 4 + n * d * 2
    qs = gaussian(3, d, 141)
    res = [check(idx, q, k, "list", on=0, label=f"1M q{j}") for j, q in enumerate(qs)]
    idx.set_screen(0)
    assert idx.hbm_bytes == n * d * 4 and idx.screen_stats()["shadow"] == 0
    for q, (s, r) in zip(qs, res):
        s2, r2 = idx.search_batch(q[None, :], k)
        assert not [x for x in _native.last_launches() if is_screen(x[0])]
        assert np.array_equal(r, r2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
    idx.set_screen(1)
    assert idx.hbm_bytes == n * d * 4 + n * d * 2
    check(idx, qs[0], k, "list", on=0, label="1M, shadow rebuilt")
    idx.release()


@pytest.mark.gpu
def test_refused_shadow_is_not_a_failure(gpu):
    lib = _native.load()
    n, d = 8000, 1536
    m = gaussian(n, d, 150)
    assert lib.svs_internal_tune(3, 1) == 0
    try:
        idx = DeviceIndex(m, device=0)
        idx.append(gaussian(500, d, 151))
        assert idx.screen_stats()["shadow"] == 0 and idx.hbm_bytes < (n + 500) * d * 4 * 1.6 and idx.n == n + 500
        check(idx, unit(np.random.default_rng(152).standard_normal(d)), 100, "off", label="shadow refused")
        idx.release()
        idx = DeviceIndex(m, device=0)            # ... and refused while an append grows it
    finally:
        assert lib.svs_internal_tune(3, 0) == 0
    idx.set_screen(1)
    assert idx.screen_stats()["shadow"] == 1
    assert lib.svs_internal_tune(3, 1) == 0
    try:
        idx.append(gaussian(6000, d, 153))        # outgrows the capacity: the new shadow is refused, the append succeeds
    finally:
        assert lib.svs_internal_tune(3, 0) == 0
    assert idx.n == n + 6000 and idx.screen_stats()["shadow"] == 0
    check(idx, unit(np.random.default_rng(154).standard_normal(d)), 100, "off", label="shadow lost in an append")
    idx.release()


@pytest.mark.gpu
def test_environment_default_off(gpu, tmp_path):
    code = ("import numpy as np\nfrom svs_amd import DeviceIndex\n"
            "m = np.random.default_rng(0).standard_normal((6000, 512), dtype=np.float32)\n"
            "i = DeviceIndex(m, device=0)\nassert i.screen_stats()['shadow'] == 0 and i.hbm_bytes == 6000 * 512 * 4\n"
            "i.set_screen(1)\nassert i.screen_stats()['shadow'] == 1\nprint('ok')\n")
    env = dict(os.environ, SVS_AMD_SCREEN="0", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


# ---- what hipcc made of the new kernels ---------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch():
    """No device needed (so this one also runs in the CPU suite): 0 scratch / 0 spills for the kernels this path adds,
    from the build's own resource report, as tests/test_kernel_resources.py reads it."""
    res = os.path.join(ROOT, "svs_amd", "lib", "build", "svs_amd.resources.txt")
    if not os.path.exists(res):
        subprocess.run(["make", "-C", os.path.join(ROOT, "svs_amd", "csrc"), "-B", "-j2"], check=True)
    with open(res) as f:
        txt = f.read()
    seen = set()
    for block in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = block.split()[0]
        fam = next((k for k in ("rescore_f32_kernel", "screen_filter_kernel", "shadow_rows_kernel") if k in name), None)
        if not fam:
            continue
        seen.add(fam)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
        spill = int(re.search(r"VGPRs Spill: (\d+)", block).group(1)) + int(re.search(r"SGPRs Spill: (\d+)", block).group(1))
        assert scratch == 0 and spill == 0, (name, scratch, spill)
    assert seen == {"rescore_f32_kernel", "screen_filter_kernel", "shadow_rows_kernel"}, seen

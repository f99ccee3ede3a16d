"""GPU: what ingest stores, bit for bit, against the CPU model of tests/ingest_model.py.

Nearly every other GPU test takes its truth from ``stored_rows`` / ``stored_query``; this file pins those.  The device
image is read with svs_internal_stored_image (plain copies, no kernel, padding columns, fp8 scales and the half shadow
included) and compared as integers, NaN canonicalised, so that -0 and +0 differ.  Every path is compared with the
model, never with a second index.  No search or score entry is called here.

fp8 codes are checked against two references that agree on the CPU (tests/test_ingest_model.py): the hand-written
e4m3fn encoder and torch's CPU float8_e4m3fn cast.
"""
import functools

import numpy as np
import pytest

import ingest_model as im
from svs_amd import DeviceIndex, _native

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "fp8")


def _same(got, exp, what):
    """Integer arrays equal; on a failure: how many elements differ and the first few (index, got, expected)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    if np.array_equal(got, exp):
        return
    bad = np.argwhere(got != exp)
    first = [(tuple(int(x) for x in i), hex(int(got[tuple(i)])), hex(int(exp[tuple(i)]))) for i in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ; (index, device, model): {first}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_image(idx, m, what, both=False, row0=0):
    """Rows [row0, row0 + len(m)) of the index hold the model image of the f32 rows m: elements, padding, fp8 scales,
    and -- where the index has one -- the half shadow.  both: the fp8 codes against torch's cast as well."""
    dtype, d, n = idx.dtype, idx.d, len(m)
    assert idx.ld == im.choose_ld(d, dtype), (what, idx.ld)
    exp_raw, exp_scales = im.image(m, dtype, idx.ld)
    raw = idx.stored_image("rows", row0, n)
    _same(im.canon_image(raw, dtype), im.canon_image(exp_raw, dtype), f"{what}: {dtype} rows")
    eb = im.ELEM_BYTES[dtype]
    assert not raw.reshape(n, idx.ld, eb)[:, d:].any(), f"{what}: padding columns are not zero"
    if dtype == "fp8":
        _same(_bits(idx.stored_image("scales", row0, n)), _bits(exp_scales), f"{what}: fp8 scales")
        if both:
            torch_raw, _ = im.image(m, dtype, idx.ld, encode=im.e4m3_encode_torch)
            _same(im.canon8(raw), im.canon8(torch_raw), f"{what}: fp8 codes against torch's cast")
    return raw


def _check_shadow(idx, m, what, row0=0):
    """The half shadow of rows [row0, row0 + len(m)) is numpy's half of the f32 rows, zero padded."""
    assert idx.dtype == "f32" and idx.screen_stats()["shadow"] == 1, what
    exp = np.zeros((len(m), idx.ld), dtype=np.uint16)
    exp[:, :idx.d] = im.half_bits(m)
    _same(im.canon16(idx.stored_image("shadow", row0, len(m))), im.canon16(exp), f"{what}: half shadow")


# ---- a. exhaustive rounding ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _half_matrix():
    m = im.half_edge_matrix(1024)
    m.setflags(write=False)
    return m


def test_f16_rounds_every_half_edge_like_numpy(gpu):
    """Every finite half, every midpoint and its f32 neighbours, both signs, overflow, inf, NaN, zeros: ~250 x 1024."""
    m = _half_matrix()
    assert 245 <= len(m) <= 255
    idx = DeviceIndex(m, dtype="f16")
    _check_image(idx, m, "half edges")
    _same(im.canon32(idx.stored_rows()), im.canon32(im.half_bits(m).view(np.float16).astype(np.float32)), "half edges: stored_rows")
    idx.release()


def test_shadow_rounds_every_half_edge_like_numpy(gpu):
    """The same matrix in an f32 index with a shadow, without what half cannot hold (those set `bad` and drop it)."""
    m = _half_matrix()
    m = np.where(np.abs(m) <= np.float32(65504.0), m, np.float32(1.0))     # (NaN compares false: replaced as well)
    idx = DeviceIndex(m)
    _check_image(idx, m, "half edges, f32")
    _check_shadow(idx, m, "half edges, f32")
    idx.release()


def test_fp8_rounds_every_e4m3_edge_at_six_scales(gpu):
    """One row per scale 2^k: 2^k * {every finite e4m3 value, every midpoint, each midpoint -+ 1 f32 ulp}, both signs,
    one column on 448 * 2^k.  Codes equal both references, the scale is 2^k -- and 2^-126 for k = -140, whose maximum
    7 * 2^-134 lies under the floor: without the floor that row is stored as NaN throughout."""
    m = im.fp8_edge_rows()
    idx = DeviceIndex(m, dtype="fp8")
    raw = _check_image(idx, m, "e4m3 edges", both=True)
    scales = idx.stored_image("scales")
    exp = np.float32([2.0 ** max(k, -126) for k in im.FP8_EDGE_KS])
    _same(_bits(scales), _bits(exp), "e4m3 edges: scales are the powers of two")
    exact = [i for i, k in enumerate(im.FP8_EDGE_KS) if k >= -100]          # (every product 2^k * value exact in f32)
    pure = im.e4m3_encode(m[im.FP8_EDGE_KS.index(0)])
    for i in exact:
        _same(raw[i, :idx.d], pure, f"e4m3 edges: k = {im.FP8_EDGE_KS[i]} stores the codes of k = 0")
    back = idx.stored_rows()
    assert np.isfinite(back).all()
    _same(im.canon32(back), im.canon32(im.decode(raw, scales, "fp8", idx.d)), "e4m3 edges: stored_rows")
    idx.release()


# ---- b. scales and geometry of the quantiser -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 65, 100, 255, 257, 1000, 1537])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantiser_scales_and_geometry(gpu, dtype, d):
    m, tags = im.edge_corpus(d)
    idx = DeviceIndex(m, dtype=dtype)
    raw = _check_image(idx, m, f"edge corpus d={d}", both=True)
    if dtype == "fp8":
        scales = idx.stored_image("scales")
        codes = raw[:, :d]
        for r, tag in enumerate(tags):
            row = m[r]
            finite = row[~np.isnan(row)]
            mx = np.float32(np.abs(finite).max()) if len(finite) else np.float32(0)
            nan_code = (codes[r] & 0x7F) == 0x7F
            if tag == "zero":
                assert scales[r] == np.float32(1.0) and not raw[r].any()
            elif tag == "nan":                              # the maximum skips it; only that element is the NaN code
                assert _bits(scales[r]) == _bits(mx / np.float32(448.0) if mx > 0 else np.float32(1.0)), (tag, r)
                assert np.array_equal(nan_code, np.isnan(row)), (tag, r)
            elif tag == "inf":                              # as the kernel stands: scale inf, the row reads back NaN
                assert np.isposinf(scales[r]) and np.array_equal(nan_code, np.isinf(row)), (tag, r)
                assert not (codes[r][~nan_code] & 0x7F).any()
                assert np.isnan(idx.stored_rows(r, 1)).all()
            elif tag == "tiny":                             # below the floor: scale 2^-126, finite, within the bound
                assert mx < im.FP8_MIN_ROW_MAX and scales[r] == np.float32(2.0 ** -126) and not nan_code.any(), (tag, r)
                back = idx.stored_rows(r, 1)[0].astype(np.float64)
                assert np.all(np.abs(back - row) <= 17.0 * float(im.FP8_MIN_ROW_MAX) / 448.0), (tag, r)
                q_raw, q_scales = im.image(row[None, :], "fp8", idx.ld)   # a query of that size: the same kernel
                _same(im.canon32(idx.stored_query(row)), im.canon32(im.decode(q_raw, q_scales, "fp8", d))[0], f"tiny query d={d} row {r}")
            else:
                assert _bits(scales[r]) == _bits(mx / np.float32(448.0)) and not nan_code.any(), (tag, r)
                assert (codes[r] & 0x7F).max() == 0x7E, (tag, r)            # the maximum sits on 448
        ok = [r for r, tag in enumerate(tags) if tag != "inf"]
        back = idx.stored_rows()[ok].astype(np.float64)
        row_max = np.fmax.reduce(np.abs(m[ok]), axis=1, initial=np.float32(0)).astype(np.float64)
        bound = 17.0 * np.maximum(row_max, float(im.FP8_MIN_ROW_MAX)) / 448.0
        keep = ~np.isnan(m[ok])
        assert np.all(np.abs(np.where(keep, back - m[ok], 0.0)) <= bound[:, None])
        assert np.array_equal(np.isnan(back), ~keep)
    idx.release()


# ---- c. every ingest path stores the same image ----------------------------------------------------------------------
def _rows(n, d, seed):
    """Gaussian rows of mixed magnitude (inside half's range), a few exact zeros of both signs."""
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal((n, d)) * np.exp2(rng.uniform(-9.0, 3.0, (n, 1)))).astype(np.float32)
    m[rng.integers(0, n, 40), rng.integers(0, d, 40)] = 0.0
    m[rng.integers(0, n, 40), rng.integers(0, d, 40)] = -0.0
    return m


def _wide(m, extra=5):
    """m on the device inside rows of d + extra floats, the extra columns NaN."""
    import torch
    w = torch.full((m.shape[0], m.shape[1] + extra), float("nan"), device="cuda:0", dtype=torch.float32)
    w[:, :m.shape[1]] = torch.from_numpy(np.array(m)).to("cuda:0")
    torch.cuda.synchronize()
    return w


def _check_all(idx, m, what):
    assert idx.n == len(m), (what, idx.n)
    _check_image(idx, m, what)
    if idx.dtype == "f32" and idx.d == 1000:
        _check_shadow(idx, m, what)                          # (ld = 1024: such an index screens, every path feeds the shadow)


PATH_N, PATH_D = 1700, 1000


@functools.lru_cache(maxsize=None)
def _path_rows():
    m = _rows(PATH_N, PATH_D, 31)
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_create_from_host(gpu, dtype):
    m = _path_rows()
    idx = DeviceIndex(m, dtype=dtype)
    _check_all(idx, m, "create")
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_append(gpu, dtype):
    m = _path_rows()
    idx = DeviceIndex(m[:600], dtype=dtype)
    idx.append(m[600:])
    _check_all(idx, m, "append")
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_device_source_with_a_wider_stride(gpu, dtype):
    m = _path_rows()
    w = _wide(m)
    idx = DeviceIndex.from_device_pointer(w.data_ptr(), 600, PATH_D, src_ld=PATH_D + 5, dtype=dtype)
    _check_all(idx, m[:600], "from_device")
    idx.append_device(w[600:].data_ptr(), PATH_N - 600, src_ld=PATH_D + 5)
    _check_all(idx, m, "append_device")
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_two_staging_commits(gpu, dtype):
    m = _path_rows()
    idx = DeviceIndex(m[:600], dtype=dtype)
    for r0, r1 in ((600, 1100), (1100, PATH_N)):             # two commits in a row: both blocks in flight
        blk = idx.staging_acquire()
        blk[:r1 - r0] = m[r0:r1]
        idx.staging_commit(r1 - r0)
    _check_all(idx, m, "staging, commits pending")           # (the read-back waits for the staging stream)
    idx.staging_finish()
    _check_all(idx, m, "staging, finished")
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_append_into_reserved_room(gpu, dtype):
    m = _path_rows()
    idx = DeviceIndex(m[:600], dtype=dtype)
    idx.reserve(PATH_N)
    held = idx.hbm_bytes
    idx.append(m[600:1000])
    idx.append(m[1000:])
    assert idx.hbm_bytes == held                             # no growth: the rows went into the reserved room
    _check_all(idx, m, "reserve + append")
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
def test_path_append_that_grows_twice(gpu, dtype):
    m = _path_rows()
    idx = DeviceIndex(m[:300], dtype=dtype)
    idx.append(m[300:400])                                   # capacity 300 -> 1474
    held = idx.hbm_bytes
    idx.append(m[400:])                                      # 1700 rows do not fit: the buffers move again
    assert idx.hbm_bytes > held
    _check_all(idx, m, "two growths")                        # the old rows survived both moves
    idx.release()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,source", [(8200, 100, "host"),       # more rows than the 2048 x 4 waves of one quantiser launch
                                        (16390, 100, "device"),    # more than 4096 x 4 waves
                                        (8193, 1025, "host")])     # two 32 MiB upload chunks, rows 0 .. 8183 in the first
def test_path_shapes_that_reach_the_loops(gpu, dtype, n, d, source):
    m = _rows(n, d, 40 + d)
    if source == "host":
        assert (d == 1025) == ((32 << 20) // (4 * d) < n)    # only the last shape takes a second 32 MiB chunk (8184 rows fill one)
        idx = DeviceIndex(m, dtype=dtype)
    else:
        w = _wide(m)
        idx = DeviceIndex.from_device_pointer(w.data_ptr(), n, d, src_ld=d + 5, dtype=dtype)
        del w
    _check_all(idx, m, f"{n} x {d} from the {source}")
    idx.release()


# ---- d. the decoder --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 100, 1537])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stored_rows_decodes_the_raw_image(gpu, dtype, d):
    m, _ = im.edge_corpus(d, seed=1)
    m = np.concatenate([m, _rows(40, d, 50 + d)])
    n = len(m)
    idx = DeviceIndex(m, dtype=dtype)
    raw = idx.stored_image("rows")
    scales = idx.stored_image("scales") if dtype == "fp8" else None
    exp = im.canon32(im.decode(raw, scales, dtype, d))
    for row0, nrows in ((0, n), (7, 20), (n - 5, 5), (13, 1), (n - 1, 1), (0, 1)):
        _same(im.canon32(idx.stored_rows(row0, nrows)), exp[row0:row0 + nrows], f"stored_rows({row0}, {nrows}) d={d}")
    for r in (0, 9, 15, 16, 17, 19, n - 3):                  # a query is stored as a one-row corpus would be (zero, NaN, inf, tiny too)
        q = m[r]
        q_raw, q_scales = im.image(q[None, :], dtype, idx.ld)
        _same(im.canon32(idx.stored_query(q)), im.canon32(im.decode(q_raw, q_scales, dtype, d))[0], f"stored_query(row {r}) d={d}")
    idx.release()


# ---- e. compaction keeps the images together -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_compaction_keeps_rows_scales_and_shadow_together(gpu, dtype):
    n, d = 3000, 512
    m = _rows(n, d, 60)
    idx = DeviceIndex(m, dtype=dtype)
    dead = np.union1d(np.arange(0, n, 7), np.arange(1400, 1600))
    idx.mask_rows(dead)
    old = idx.compact()
    live = np.setdiff1d(np.arange(n), dead)
    assert np.array_equal(old, live) and idx.n == len(live) and idx.n_masked == 0
    _check_image(idx, m[live], "compacted")
    if dtype == "f32":
        _check_shadow(idx, m[live], "compacted")
        rows = idx.stored_image("rows").view(np.float32)
        _same(im.canon16(idx.stored_image("shadow")), im.canon16(im.half_bits(rows)), "compacted: shadow[p] == half(rows[p])")
    extra = _rows(100, d, 61)
    idx.append(extra)
    both = np.concatenate([m[live], extra])
    assert idx.n == len(both)
    _check_image(idx, both, "compacted + append")
    if dtype == "f32":
        _check_shadow(idx, both, "compacted + append")
    idx.release()


# ---- f. shadow statistics --------------------------------------------------------------------------------------------
def _shadow_truth(m):
    """(A, B, C) in f64: max over rows of ||m - half(m)||, ||half(m)||, ||m||."""
    x = m.astype(np.float64)
    h = m.astype(np.float16).astype(np.float64)
    norm = lambda a: np.sqrt((a * a).sum(axis=1)).max()
    return norm(x - h), norm(h), norm(x)


def test_shadow_statistics_bound_the_truth_from_above(gpu):
    """truth <= stat (each statistic is rounded up: the screening bound relies on it) and stat <= truth * 1.002:
    SCREEN_UP = 1.001 times the 2.5e-4 screen.h states for an f32 sum of at most 4096 squares, rounded up."""
    n, d = 3000, 512
    rng = np.random.default_rng(70)
    unit = rng.standard_normal((n + 500, d))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    m = (unit * 10.0 ** rng.uniform(-1.0, 1.0, (n + 500, 1))).astype(np.float32)
    m[n:] *= np.float32(1.5)                                 # the appended rows raise every statistic
    idx = DeviceIndex(m[:n])

    def check(rows, what, upper=True):
        st = idx.screen_stats()
        assert st["shadow"] == 1, what
        for name, truth in zip("ABC", _shadow_truth(rows)):
            print(f"{what}: {name} = {st[name]!r}, truth {truth!r}, ratio {st[name] / truth:.7f}")
            assert truth <= st[name], (what, name, truth, st[name])
            assert not upper or st[name] <= truth * 1.002, (what, name, truth, st[name])

    check(m[:n], "create")
    idx.append(m[n:])
    check(m, "append")
    norms = np.linalg.norm(m.astype(np.float64), axis=1)
    dead = np.argsort(norms)[-300:]                          # the largest rows go: the statistics are monotone, they stay
    idx.mask_rows(dead)
    idx.compact()
    check(np.delete(m, dead, axis=0), "compacted", upper=False)
    idx.release()


# ---- g. the hook's errors --------------------------------------------------------------------------------------------
def test_stored_image_errors(gpu):
    import ctypes as C
    lib = _native.load()
    call = lambda h, what, row0, nrows, buf, cap: lib.svs_internal_stored_image(h, what, row0, nrows, buf, cap)
    m = _rows(50, 512, 80)
    buf = np.zeros(50 * 512 * 4 + 64, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    f32, f16, fp8 = DeviceIndex(m), DeviceIndex(m, dtype="f16"), DeviceIndex(m, dtype="fp8")
    plain = DeviceIndex(m[:, :100])                          # ld = 100: no shadow
    assert f32.screen_stats()["shadow"] == 1 and plain.screen_stats()["shadow"] == 0
    U, I = _native.SVS_ERR_UNSUPPORTED, _native.SVS_ERR_INVALID
    assert call(f32._handle(), 1, 0, 1, p, buf.nbytes) == U and call(f16._handle(), 1, 0, 1, p, buf.nbytes) == U
    assert call(f16._handle(), 2, 0, 1, p, buf.nbytes) == U and call(fp8._handle(), 2, 0, 1, p, buf.nbytes) == U
    assert call(plain._handle(), 2, 0, 1, p, buf.nbytes) == U
    assert call(None, 0, 0, 1, p, buf.nbytes) == I and call(f32._handle(), 0, 0, 1, None, buf.nbytes) == I
    assert call(f32._handle(), 3, 0, 1, p, buf.nbytes) == I and call(f32._handle(), -1, 0, 1, p, buf.nbytes) == I
    for row0, nrows in ((-1, 1), (0, 51), (50, 1), (49, 2), (0, -1), (2 ** 62, 2 ** 62)):
        assert call(f32._handle(), 0, row0, nrows, p, buf.nbytes) == I, (row0, nrows)
    assert call(f32._handle(), 0, 0, 50, p, 50 * 512 * 4 - 1) == I and call(f32._handle(), 0, 0, 50, p, 50 * 512 * 4) == 0
    assert call(fp8._handle(), 1, 0, 50, p, 199) == I and call(fp8._handle(), 1, 0, 50, p, 200) == 0
    assert call(f32._handle(), 2, 0, 50, p, 50 * 512 * 2 - 1) == I and call(f32._handle(), 2, 0, 50, p, 50 * 512 * 2) == 0
    assert call(f32._handle(), 0, 50, 0, p, 0) == 0          # an empty range at the end is a range
    assert not buf[50 * 512 * 4:].any()                      # nothing was written past an image
    with pytest.raises(NotImplementedError):
        f16.stored_image("scales")
    with pytest.raises(ValueError):
        f16.stored_image("rows", 10, 41)
    for idx in (f32, f16, fp8, plain):
        idx.release()

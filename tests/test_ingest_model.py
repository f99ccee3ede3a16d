"""The CPU model of the stored image (tests/ingest_model.py) against references that are not the model: torch's CPU
float8_e4m3fn cast for the hand-written e4m3 encoder, the format's definition for the value table, and hand-computed
rows for the recipe.  No GPU."""
import numpy as np
import pytest

import ingest_model as im


def _both_signs(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([v, -v])


def test_e4m3_table_is_the_ocp_format():
    t = im.E4M3_VALUES
    assert t.shape == (256,) and np.isnan(t[0x7F]) and np.isnan(t[0xFF]) and np.isfinite(np.delete(t, [0x7F, 0xFF])).all()
    assert t[0x00] == 0 and np.signbit(t[0x80]) and t[0x80] == 0
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9 and t[0x08] == 2.0 ** -6   # subnormals, then the first normal
    assert t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0xFE] == -448.0
    assert np.all(np.diff(t[:127]) > 0) and np.array_equal(t[128:255], -t[:127])


def test_e4m3_table_matches_torch():
    import torch
    got = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert np.array_equal(im.canon32(got), im.canon32(im.E4M3_VALUES))


def test_e4m3_encoder_matches_torch_on_every_edge():
    """Every finite value, every midpoint between neighbours (464 included), each midpoint -+ 1 f32 ulp, both signs;
    then the same set scaled by powers of two is covered by the quantiser tests on the device."""
    import torch  # noqa: F401
    v = _both_signs(im.e4m3_edge_values(top=True))
    assert v.shape == (2 * (127 + 3 * 127),)
    mine, theirs = im.e4m3_encode(v), im.e4m3_encode_torch(v)
    assert np.array_equal(mine, theirs)            # (the NaN code carries the sign in both)
    extra = np.array([np.inf, -np.inf, np.nan, 480.0, 1e30, -1e30, 2.0 ** -149, -2.0 ** -149, 2.0 ** -10, 2.0 ** -11], dtype=np.float32)
    assert np.array_equal(im.canon8(im.e4m3_encode(extra)), im.canon8(im.e4m3_encode_torch(extra)))


def test_e4m3_encoder_rounds_by_hand():
    enc = lambda *x: im.e4m3_encode(np.array(x, dtype=np.float32)).tolist()
    assert enc(0.0, -0.0, 448.0, -448.0, 1.0) == [0x00, 0x80, 0x7E, 0xFE, 0x38]
    assert enc(2.0 ** -10, -2.0 ** -10) == [0x00, 0x80]                       # halfway to the first subnormal: even is 0
    assert enc(3 * 2.0 ** -10, 1.0625, 1.1875) == [0x02, 0x38, 0x3A]          # ties go to the even code
    assert enc(464.0, np.nextafter(np.float32(464.0), np.float32(np.inf)), np.inf, -np.inf) == [0x7E, 0x7F, 0x7F, 0xFF]
    assert im.canon8(im.e4m3_encode(np.array([np.nan], dtype=np.float32))).tolist() == [0x7F]
    codes = np.arange(256, dtype=np.uint8)
    finite = (codes & 0x7F) != 0x7F
    assert np.array_equal(im.e4m3_encode(im.e4m3_decode(codes[finite])), codes[finite])   # a round trip keeps every code


def test_e4m3_encoder_random_matches_torch():
    import torch  # noqa: F401
    rng = np.random.default_rng(5)
    v = (rng.standard_normal(200000) * np.exp2(rng.integers(-14, 9, 200000))).astype(np.float32)
    assert np.array_equal(im.e4m3_encode(v), im.e4m3_encode_torch(v))


def test_half_edges_cover_every_finite_half():
    v = im.half_edge_values()
    assert v.shape == (4 * 0x7C00,) and v.dtype == np.float32
    bits = im.half_bits(v[:0x7C00])
    assert np.array_equal(bits, np.arange(0x7C00, dtype=np.uint16))           # the values themselves are kept
    mid = v[0x7C00:2 * 0x7C00]
    lo = np.arange(0x7C00, dtype=np.uint16)
    assert np.array_equal(im.half_bits(mid), lo + (lo & 1))                   # a midpoint goes to the even neighbour
    assert np.array_equal(im.half_bits(v[2 * 0x7C00:3 * 0x7C00]), lo)         # one ulp below it: down
    assert np.array_equal(im.half_bits(v[3 * 0x7C00:]), lo + 1)               # one ulp above it: up (0x7c00 is inf)
    assert im.half_bits(np.float32([65504, 65519.996, 65520, 1e5, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23)])).tolist() == \
        [0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0x0001, 0x0000, 0x0001]


def test_choose_ld_cases():
    # (d, f32, f16, fp8): worked from the three rules by hand
    for d, a, b, c in [(1, 4, 8, 16), (3, 4, 8, 16), (64, 64, 64, 64), (100, 100, 104, 112), (512, 512, 512, 512),
                       (1000, 1024, 1024, 1024), (1025, 1056, 1088, 1152), (1536, 1536, 1536, 2048 - 512), (1537, 1568, 1600, 1664)]:
        assert (im.choose_ld(d, "f32"), im.choose_ld(d, "f16"), im.choose_ld(d, "fp8")) == (a, b, c), d
    for dtype in im.ELEM_BYTES:
        for d in range(1, 4200):
            ld = im.choose_ld(d, dtype)
            assert ld >= d and ld * im.ELEM_BYTES[dtype] % 16 == 0 and ld * 8 <= (d + 16 // im.ELEM_BYTES[dtype] - 1) * 9


def test_image_f32_f16_layout():
    m = np.array([[1.0, -0.0, 65520.0], [2.0 ** -25, np.nan, -np.inf]], dtype=np.float32)
    raw, s = im.image(m, "f32", 4)
    assert s is None and raw.shape == (2, 16) and raw.view(np.uint32)[:, :3].tolist() == m.view(np.uint32).tolist()
    assert raw.view(np.uint32)[:, 3].tolist() == [0, 0]
    raw, s = im.image(m, "f16", 8)
    assert s is None and raw.shape == (2, 16)
    assert im.canon_image(raw, "f16").tolist() == [[0x3C00, 0x8000, 0x7C00, 0, 0, 0, 0, 0], [0, 0x7E00, 0xFC00, 0, 0, 0, 0, 0]]
    assert np.array_equal(im.canon32(im.decode(raw, None, "f16", 3)), im.canon32(np.float32([[1, -0.0, np.inf], [0, np.nan, -np.inf]])))


def test_image_fp8_recipe_by_hand():
    m = np.array([[896.0, -448.0, 0.0, -0.0, 2.0],            # scale 2: codes of 448, -224, 0, -0, 1
                  [0.0, 0.0, 0.0, 0.0, 0.0],                  # all zero: scale 1
                  [np.nan, 3.5, -7.0, 0.0, 0.0],              # the NaN is not the maximum: scale 7 / 448 = 2^-6
                  [np.inf, 1.0, -1.0, 0.0, -0.0]],            # scale inf, 1 / scale = 0: zeros, and inf * 0 = NaN
                 dtype=np.float32)
    raw, s = im.image(m, "fp8", 16)
    assert raw.shape == (4, 16) and not raw[:, 5:].any()
    assert s.view(np.uint32).tolist() == np.float32([2.0, 1.0, 2.0 ** -6, np.inf]).view(np.uint32).tolist()
    assert im.canon8(raw[:, :5]).tolist() == [[0x7E, 0xF6, 0x00, 0x80, 0x38], [0, 0, 0, 0, 0],
                                              [0x7F, 0x76, 0xFE, 0x00, 0x00], [0x7F, 0x00, 0x80, 0x00, 0x80]]
    back = im.decode(raw, s, "fp8", 5)
    assert np.array_equal(im.canon32(back[:3]), im.canon32(np.float32([[896, -448, 0, -0.0, 2], [0] * 5, [np.nan, 3.5, -7, 0, 0]])))
    assert np.isnan(back[3]).all()                            # 0 * inf: the whole row reads back as NaN
    raw_t, s_t = im.image(m, "fp8", 16, encode=im.e4m3_encode_torch)
    assert np.array_equal(im.canon8(raw), im.canon8(raw_t)) and np.array_equal(s, s_t)


TINY = [1.3e-36, 1e-37, 1e-40, 2.0 ** -149]


def _tiny_rows():
    rows = []
    for mx in TINY:
        r = np.zeros(8, dtype=np.float32)
        r[0], r[1], r[2], r[5] = mx, -np.float32(mx) / 2, np.float32(mx) / 4, -0.0
        rows.append(r)
    return np.stack(rows)


def test_tiny_rows_overflowed_before_the_floor():
    """The recipe without the floor (scale = max / 448, inv = 1 / scale): below max|x| = 448 / FLT_MAX the inverse
    overflows to inf, the non-zero elements become the NaN code and the zeros 0 * inf = NaN: the row reads back as NaN."""
    m = _tiny_rows()
    raw, s = im.image(m, "fp8", 16, floor=0.0)
    assert np.all((raw[:, :8] & 0x7F) == 0x7F) and np.isnan(im.decode(raw, s, "fp8", 8)).all()
    ok = np.zeros((2, 8), dtype=np.float32)
    ok[0, 0], ok[1, 0] = 1.4e-36, 6e-36                       # just above the overflow; above the floor
    raw0, s0 = im.image(ok, "fp8", 16, floor=0.0)
    raw1, s1 = im.image(ok, "fp8", 16)
    assert raw0[:, 0].tolist() == [0x7E, 0x7E] and not raw0[:, 1:].any()
    assert np.array_equal(raw0[1], raw1[1]) and s0[1] == s1[1]                  # the floor leaves that row alone
    assert raw1[0, 0] == 0x6F and s1[0] == np.float32(2.0 ** -126)             # 1.4e-36 * 2^126 = 119.1 -> 120


def test_tiny_rows_with_the_floor():
    """With the floor every finite row reads back finite, zeros as zeros, within 17 * max(mx, 7 * 2^-120) / 448."""
    m = _tiny_rows()
    raw, s = im.image(m, "fp8", 16)
    assert s.view(np.uint32).tolist() == [np.float32(2.0 ** -126).view(np.uint32)] * 4
    back = im.decode(raw, s, "fp8", 8)
    assert np.isfinite(back).all()
    assert np.array_equal(im.canon32(back[:, 3:]), im.canon32(m[:, 3:]))        # zeros, and the sign of -0
    bound = 17.0 * max(float(np.abs(m).max()), float(im.FP8_MIN_ROW_MAX)) / 448.0
    assert np.max(np.abs(back.astype(np.float64) - m.astype(np.float64))) <= bound
    assert raw[0, 0] == im.e4m3_encode(np.float32([np.float32(1.3e-36) * np.float32(2.0 ** 126)]))[0]


def test_floor_changes_no_row_at_or_above_it():
    """Rows with max|x| >= 7 * 2^-120 store what they stored before the floor: same scale bits, same codes."""
    rng = np.random.default_rng(11)
    mags = np.exp2(rng.uniform(-118.0, 120.0, 400)).astype(np.float32)
    m = (rng.standard_normal((400, 33)) * mags[:, None]).astype(np.float32)
    m[0] = 0
    m[0, 7] = im.FP8_MIN_ROW_MAX                               # exactly the floor
    m = m[np.abs(m).max(axis=1) >= im.FP8_MIN_ROW_MAX]
    assert len(m) > 390
    a, sa = im.image(m, "fp8", 48, floor=0.0)
    b, sb = im.image(m, "fp8", 48)
    assert np.array_equal(a, b) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    assert sb[0] == np.float32(2.0 ** -126)
    back = im.decode(b, sb, "fp8", 33).astype(np.float64)
    assert np.all(np.abs(back - m) <= 17.0 * np.abs(m).max(axis=1, keepdims=True).astype(np.float64) / 448.0)


def test_gpu_corpora_show_the_overflow_without_the_floor():
    """The rows tests/test_ingest_image_gpu.py requires to read back finite are exactly those the recipe without the
    floor stores as NaN: the k = -140 row of the e4m3 edge matrix and the `tiny` rows of the edge corpus."""
    m = im.fp8_edge_rows()
    assert m.shape == (6, 1 + 2 * (127 + 3 * 126)) and np.array_equal(np.abs(m).max(axis=1), m[:, 0])
    for floor, nan_rows in ((0.0, [0]), (im.FP8_MIN_ROW_MAX, [])):
        raw, s = im.image(m, "fp8", 1024, floor=floor)
        back = im.decode(raw, s, "fp8", m.shape[1])
        assert np.flatnonzero(np.isnan(back).any(axis=1)).tolist() == nan_rows
        assert np.flatnonzero(np.isnan(back).all(axis=1)).tolist() == nan_rows
        assert s[1:].tolist() == [2.0 ** k for k in im.FP8_EDGE_KS[1:]]
    assert s[0] == np.float32(2.0 ** -126)
    for d in (1, 3, 100):
        m, tags = im.edge_corpus(d)
        tiny = [r for r, t in enumerate(tags) if t == "tiny"]
        assert len(tiny) == 4 and [float(np.abs(m[r]).max()) for r in tiny] == [float(np.float32(x)) for x in im.FP8_TINY_MAXIMA]
        finite_rows = [r for r, t in enumerate(tags) if t not in ("nan", "inf")]
        raw, s = im.image(m, "fp8", im.choose_ld(d, "fp8"), floor=0.0)
        bad = np.flatnonzero(np.isnan(im.decode(raw, s, "fp8", d)[finite_rows]).any(axis=1))
        assert [finite_rows[i] for i in bad] == tiny
        raw, s = im.image(m, "fp8", im.choose_ld(d, "fp8"))
        assert np.isfinite(im.decode(raw, s, "fp8", d)[finite_rows]).all()


def test_decode_is_one_f32_multiply():
    codes = np.arange(256, dtype=np.uint8)[None, :].repeat(3, axis=0)
    s = np.float32([2.0 ** -126, 3.3e-5, 1.7e30])
    got = im.decode(codes, s, "fp8", 256)
    exp = np.stack([(im.E4M3_VALUES.astype(np.float64) * float(x)).astype(np.float32) for x in s])   # exact product, one rounding
    assert np.array_equal(im.canon32(got), im.canon32(exp))

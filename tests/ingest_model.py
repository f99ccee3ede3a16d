"""CPU model of what ingest stores in HBM (tests/test_ingest_image_gpu.py compares the device with it bit for bit).

``image`` is the byte image of a corpus as svs_index_create / append / staging leave it: rows of ``ld`` elements, the
columns from ``d`` on zero, and for fp8 one f32 scale per row.  ``decode`` is what ``stored_rows`` must make of such an
image.  Nothing here calls the library: f32 is a copy, f16 is numpy's float16 cast (round to nearest even), and fp8 is
the recipe at the top of svs_amd/csrc/fp8.h evaluated in numpy f32 with a hand-written e4m3fn encoder (the 256-entry
value table, rounding by midpoints).  ``e4m3_encode_torch`` is the same cast through torch's CPU float8_e4m3fn:
tests/test_ingest_model.py checks the two against each other on every value where they could part.
"""
import numpy as np

FP8_MAX = np.float32(448.0)
# Floor under a row's maximum: 7 * 2^-120, so that the scale is never below 2^-126 and 1 / scale never above 2^126.
FP8_MIN_ROW_MAX = np.float32(7.0 * 2.0 ** -120)
ELEM_BYTES = {"f32": 4, "f16": 2, "fp8": 1}
E4M3_NAN = 0x7F


def _e4m3_table() -> np.ndarray:
    t = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9                     # subnormals: m / 8 * 2^-6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t.astype(np.float32)                   # (every value is exact in f32)


E4M3_VALUES = _e4m3_table()                                   # code -> value; 0x7f and 0xff are NaN
E4M3_POS = E4M3_VALUES[:127].astype(np.float64)               # codes 0x00 .. 0x7e: 0 .. 448, ascending
# E4M3_MID[i]: halfway between codes i and i + 1; the last one (464) lies between 448 and the 480 the format lacks
E4M3_MID = (np.append(E4M3_POS[1:], 480.0) + E4M3_POS) / 2.0


def e4m3_encode(x) -> np.ndarray:
    """f32 -> e4m3fn codes (u8), round to nearest, ties to the even code.  Above 464 (inf included) and NaN: the NaN
    code with the sign of x.  The sign of zero, and of what rounds to zero, is kept."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x).astype(np.float64)
    nan = np.isnan(a)
    a0 = np.where(nan, 0.0, a)
    code = np.searchsorted(E4M3_MID, a0, side="left")         # midpoints strictly below |x|
    tie = (code < 127) & (E4M3_MID[np.minimum(code, 126)] == a0)
    code = np.where(tie & (code % 2 == 1), code + 1, code)    # on a midpoint: the even neighbour
    code = np.where(nan, E4M3_NAN, code).astype(np.uint8)     # (127 midpoints below |x|: the NaN code already)
    return code | (np.signbit(x).astype(np.uint8) << 7)


def e4m3_encode_torch(x) -> np.ndarray:
    """The same cast through torch's CPU float8_e4m3fn."""
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    return torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_decode(code) -> np.ndarray:
    return E4M3_VALUES[np.asarray(code, dtype=np.uint8)]


def canon8(code) -> np.ndarray:
    """e4m3 codes with both NaN codes as 0x7f (so that -0 and +0 still differ)."""
    code = np.asarray(code, dtype=np.uint8)
    return np.where((code & 0x7F) == E4M3_NAN, np.uint8(E4M3_NAN), code)


def canon16(bits) -> np.ndarray:
    """Half bit patterns with every NaN as 0x7e00."""
    bits = np.asarray(bits, dtype=np.uint16)
    return np.where((bits & 0x7FFF) > 0x7C00, np.uint16(0x7E00), bits)


def canon32(a) -> np.ndarray:
    """f32 values as bit patterns with every NaN as 0x7fc00000 (test_combined_gpu._canon)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def half_bits(m) -> np.ndarray:
    """f32 -> IEEE half bit patterns (u16), round to nearest even, overflow to inf."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(m, dtype=np.float32).astype(np.float16).view(np.uint16)


def choose_ld(d: int, dtype: str) -> int:
    """Row stride in elements (the comment above choose_ld in svs_amd.hip): rows are 16-byte aligned; a whole number of
    1 KiB wave loads when that costs at most an eighth more than the tight stride, else whole 128-byte lines under the
    same condition, else tight."""
    align = 16 // ELEM_BYTES[dtype]
    tight = -(-d // align) * align
    if d <= 0:
        return tight
    wave, line = 64 * align, 8 * align
    waved, lined = -(-d // wave) * wave, -(-d // line) * line
    if waved * 8 <= tight * 9:
        return waved
    if lined * 8 <= tight * 9:
        return lined
    return tight


def fp8_scales(m, floor=FP8_MIN_ROW_MAX) -> np.ndarray:
    """One f32 scale per row: max|row| / 448, the maximum taken without the NaN elements and not below ``floor``;
    1 for a row whose maximum is 0.  ``floor=0`` is the recipe before the floor was introduced."""
    m = np.asarray(m, dtype=np.float32)
    mx = np.fmax.reduce(np.abs(m), axis=1, initial=np.float32(0.0)).astype(np.float32)   # (fmax skips NaN, like fmaxf)
    with np.errstate(over="ignore"):
        return np.where(mx > 0, np.fmax(mx, np.float32(floor)) / FP8_MAX, np.float32(1.0)).astype(np.float32)


def image(m, dtype: str, ld: int, floor=FP8_MIN_ROW_MAX, encode=e4m3_encode):
    """(raw u8 [n][ld * element bytes], scales f32 [n] or None): the stored image of the f32 rows ``m``."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    n, d = m.shape
    assert ld >= d
    if dtype == "f32":
        out = np.zeros((n, ld), dtype=np.uint32)
        out[:, :d] = m.view(np.uint32)
        return out.view(np.uint8), None
    if dtype == "f16":
        out = np.zeros((n, ld), dtype=np.uint16)
        out[:, :d] = half_bits(m)
        return out.view(np.uint8), None
    assert dtype == "fp8"
    scales = fp8_scales(m, floor)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = (np.float32(1.0) / scales).astype(np.float32)
        v = (m * inv[:, None]).astype(np.float32)             # one f32 multiply per element
    out = np.zeros((n, ld), dtype=np.uint8)
    out[:, :d] = encode(v)
    return out, scales


def decode(raw, scales, dtype: str, d: int) -> np.ndarray:
    """The f32 rows ``stored_rows`` must return for a raw image: columns < d; f16 widened; fp8 value * scale in f32."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if dtype == "f32":
        return raw.view(np.float32)[:, :d].copy()
    if dtype == "f16":
        return raw.view(np.float16)[:, :d].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (e4m3_decode(raw[:, :d]) * np.asarray(scales, dtype=np.float32)[:, None]).astype(np.float32)


def canon_image(raw, dtype: str) -> np.ndarray:
    """A raw image as element bit patterns with NaN canonicalised (f32 is compared as it is: a copy keeps payloads)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if dtype == "f32":
        return raw.view(np.uint32)
    if dtype == "f16":
        return canon16(raw.view(np.uint16))
    return canon8(raw)


# ---- the values at which a rounding can go wrong ---------------------------------------------------------------------
def _around(mid64) -> np.ndarray:
    """f32: each midpoint, and its two f32 neighbours."""
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    return np.concatenate([mid, np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))])


def e4m3_edge_values(top: bool = False) -> np.ndarray:
    """Non-negative f64: every finite e4m3 value, every midpoint between neighbours and each midpoint -+ 1 f32 ulp.
    ``top``: also around 464, the edge between 448 and the NaN code (not reachable by a quantised row)."""
    mids = E4M3_MID if top else E4M3_MID[:-1]
    return np.concatenate([E4M3_POS, _around(mids).astype(np.float64)])


FP8_EDGE_KS = (-140, -126, -100, -12, 0, 100)


def fp8_edge_rows(ks=FP8_EDGE_KS) -> np.ndarray:
    """One f32 row per k: 2^k * {448, then every e4m3 edge value in both signs}, so that the row's scale is 2^k
    (2^-126 under the floor for k < -126).  Products that f32 cannot hold exactly (k <= -126) are rounded: the model
    quantises the f32 row it is given."""
    v = e4m3_edge_values()
    base = np.concatenate([[448.0], v, -v])
    with np.errstate(under="ignore"):
        return np.stack([(base * 2.0 ** k).astype(np.float32) for k in ks])


FP8_TINY_MAXIMA = (1.3e-36, 1e-37, 1e-40, 2.0 ** -149)        # row maxima below 448 / FLT_MAX: 1 / (max / 448) overflows


def edge_corpus(d: int, seed: int = 0):
    """(rows f32 [n][d], tags): the rows at which the quantiser's max reduction and scale can go wrong.  Magnitudes
    from 2^-100 to 2^100 that are no powers of two; the row maximum in column 0, d - 1, 63, 64, negative, and twice with
    opposite signs; an all-zero row; a NaN element; an inf element; maxima below 448 / FLT_MAX."""
    rng = np.random.default_rng(7000 + 13 * d + seed)
    rows, tags = [], []

    def add(r, tag):
        with np.errstate(under="ignore"):
            rows.append(np.asarray(r, dtype=np.float64).astype(np.float32))
        tags.append(tag)

    for e in np.linspace(-100.0, 100.0, 9):
        add(rng.standard_normal(d) * 1.37 * 2.0 ** e, "magnitude")
    for tag, cols, signs in (("max first", [0], [1]), ("max last", [d - 1], [1]), ("max 63", [min(63, d - 1)], [1]),
                             ("max 64", [min(64, d - 1)], [1]), ("max negative", [d // 2], [-1]),
                             ("max twice", [0, d - 1], [1, -1])):
        r = np.clip(rng.standard_normal(d), -3.0, 3.0) * 0.11
        for c, s in zip(cols, signs):
            r[c] = s * 5.3
        add(r, tag)
    add(np.zeros(d), "zero")
    r = rng.standard_normal(d) * 0.7
    r[d // 3] = np.nan
    add(r, "nan")
    r = rng.standard_normal(d)
    r[d - 1] = np.inf
    add(r, "inf")
    for mx in FP8_TINY_MAXIMA:
        r = rng.uniform(-1.0, 1.0, d) * mx
        r[d // 2] = mx
        add(r, "tiny")
    return np.stack(rows), tags


def half_edge_values() -> np.ndarray:
    """Non-negative f32: every finite half value h, mid(h, next) and the midpoint -+ 1 f32 ulp (the last midpoint,
    65520, lies between 65504 and the 65536 half lacks: it and what is above round to inf)."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mids = (np.append(h[1:], 65536.0) + h) / 2.0
    return np.concatenate([h.astype(np.float32), _around(mids)])


def half_edge_matrix(width: int = 1024) -> np.ndarray:
    """The half edge values in both signs, then the overflow edge, inf, NaN, the zeros and the smallest subnormal's
    edge once more by name, as rows of ``width`` (the last row filled up with 1.0)."""
    v = half_edge_values()
    extras = np.float32([65504.0, 65519.996, 65520.0, 1e5, np.inf, -np.inf, np.nan, 0.0, -0.0, 2.0 ** -24, 2.0 ** -25,
                         2.0 ** -25 * (1 + 2.0 ** -23)])
    allv = np.concatenate([v, -v, extras])
    fill = np.ones(-len(allv) % width, dtype=np.float32)
    return np.concatenate([allv, fill]).reshape(-1, width)

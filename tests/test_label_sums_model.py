"""CPU: the model of svs_index_label_sums (tests/label_sums_model.py) -- that ``replay`` is the exact sum on the plain
test data, and that the WIDE data gives the GPU comparison teeth: another chunk length, another row order or one long
chain changes at least one f64 element, while every variant stays within the rounding bound of the exact sum."""
import numpy as np
import pytest

import label_sums_model as lm

N = 4099
SEED = 20263


def _fp8_like(x):
    """Values shaped like an fp8 index's stored rows: per row scale = max |x| / 448 in f32, x / scale rounded to four
    significant bits (e4m3's grid, quantum 2^-9 below 2^-6), times the scale as one f32 product."""
    x = np.asarray(x, dtype=np.float32)
    scale = (np.abs(x).max(axis=1) / np.float32(448.0)).astype(np.float32)
    v = (x / scale[:, None]).astype(np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -6)))
    q = np.clip(np.round(v / np.exp2(e - 3)) * np.exp2(e - 3), -448.0, 448.0).astype(np.float32)
    return q * scale[:, None]


def _stored_like(x, kind):
    if kind == "f16":           # the values an f16 index stores: rounded to half (exactly representable in f32)
        return x.astype(np.float16).astype(np.float32)
    return _fp8_like(x) if kind == "fp8" else x


def _case(d, kind):
    rng = np.random.default_rng(SEED + d)
    plain, wide = lm.unit(rng, N, d), lm.wide(rng, N, d)
    lab = rng.integers(0, 3, size=N).astype(np.uint32)
    return _stored_like(plain, kind), (None if kind == "f16" else _stored_like(wide, kind)), lab      # (2^20 is no half)


CASES = [(d, kind) for d in (64, 100) for kind in ("f32", "f16", "fp8")]
WIDE_CASES = [(d, kind) for d in (64, 100) for kind in ("f32", "fp8")]


@pytest.mark.parametrize("d,kind", CASES)
def test_replay_is_the_exact_sum_on_plain_data(d, kind):
    plain, _, lab = _case(d, kind)
    got, counts = lm.replay(plain, lab, None, [0, 1, 2])
    want, wcounts = lm.exact(plain, lab, None, [0, 1, 2])
    assert lm.same_bits(got, want) and np.array_equal(counts, wcounts) and counts.sum() == N
    assert np.array_equal(counts, np.bincount(lab, minlength=3))
    # and so no variant of the order can differ here
    for kw in (dict(chunk=128), dict(order=lambda r: r[::-1]), dict(chunk=None)):
        assert lm.same_bits(lm.replay(plain, lab, None, [0, 1, 2], **kw)[0], want)


@pytest.mark.parametrize("d,kind", WIDE_CASES)
def test_wide_data_tells_orders_apart(d, kind):
    _, wide, lab = _case(d, kind)
    labels = [0, 1, 2]
    ref, counts = lm.replay(wide, lab, None, labels)
    want, _ = lm.exact(wide, lab, None, labels)
    # m 2^-53 sum |x|: m - 1 additions (chunked: fewer per chain, plus the fold), each off by at most half an ulp of a
    # partial sum, which is at most sum |x|
    absum = np.stack([np.abs(wide[lab == l].astype(np.float64)).sum(axis=0) for l in labels])
    bound = counts[:, None] * 2.0 ** -53 * absum
    assert (np.abs(ref - want) <= bound).all()
    for name, kw in (("chunk 128", dict(chunk=128)), ("reversed", dict(order=lambda r: r[::-1])), ("one chain", dict(chunk=None))):
        other, ocounts = lm.replay(wide, lab, None, labels, **kw)
        assert np.array_equal(ocounts, counts)
        differ = int((other.view(np.uint64) != ref.view(np.uint64)).any(axis=0).sum())
        print(f"d={d} {kind} {name}: {differ} of {d} columns differ from the definition's order")
        assert differ >= 1, f"{name}: the WIDE data cannot tell this order from the definition's"
        assert (np.abs(other - want) <= bound).all()


def test_empty_labels_repeats_and_live_mask():
    rng = np.random.default_rng(5)
    x = lm.unit(rng, 700, 8)
    lab = rng.integers(0, 4, size=700).astype(np.uint32) * 10          # labels 0, 10, 20, 30
    live = rng.random(700) > 0.2
    labels = [20, 7, 20, 0, 4000000000, 30, 20]
    s, c = lm.replay(x, lab, live, labels)
    assert s.shape == (7, 8) and c.dtype == np.int64
    assert c[1] == 0 and c[4] == 0 and not s[1].any() and not s[4].any()
    assert lm.same_bits(s[0], s[2]) and lm.same_bits(s[0], s[6]) and c[0] == c[2] == c[6]
    for j, l in enumerate(labels):
        rows = np.flatnonzero((lab == l) & live)
        assert c[j] == len(rows)
        assert np.allclose(s[j], x[rows].astype(np.float64).sum(axis=0), rtol=0, atol=1e-12)
    # a label's answer does not depend on the other labels of the set
    assert lm.same_bits(lm.replay(x, lab, live, [30])[0][0], s[5])
    # chunk edges: exactly chunk rows is one chunk, one more is two
    one = np.ones((257, 3), dtype=np.float32)
    s, c = lm.replay(one, np.zeros(257, dtype=np.uint32), None, [0])
    assert c[0] == 257 and (s == 257.0).all()
    m = lm.means(s, c)
    assert (m == 1.0).all() and not lm.means(np.zeros((2, 3)), np.zeros(2, dtype=np.int64)).any()


def test_never_negative_zero():
    x = np.full((5, 4), -0.0, dtype=np.float32)
    x[:, 1] = [1.0, -1.0, 2.5, -2.5, -0.0]          # cancels to zero: +0.0 under round-to-nearest
    lab = np.zeros(5, dtype=np.uint32)
    for kw in (dict(), dict(chunk=2), dict(chunk=None)):
        s, c = lm.replay(x, lab, None, [0, 9], **kw)
        assert c.tolist() == [5, 0]
        assert not np.signbit(s).any() and not s.any()
    e, _ = lm.exact(x, lab, None, [0, 9])
    assert not e.any()

"""The coherent families of certificate_data.py and its float64 model, without a device.

Two things are pinned here so that the GPU tests (test_gpu_certificate_layouts.py) mean what they say: the generators
deliver exactly the bit patterns they promise, and on those patterns the documented budget is nearly used up
by exact arithmetic on the rounded operands -- so a kernel that reads another operand than the layout's rounding, or a budget
a few per cent tighter, fails there.  The thresholds: 1.0 is the certificate's own condition; 0.9 says "this data is the
worst case" (the Cauchy-Schwarz limit is 1 / 1.014 less the (c_acc + eps) |q||d| share, 0.976 at d = 64).
"""
import zlib

import numpy as np
import pytest

from certificate_data import (COHERENT_QUERIES, FAMILIES, bf16_half_up, bf16_rne, bf16_truncate, coherent, make_case,
                              model_ratios, tie_free)

N = 600
METRICS = [0, 1, 2]


def case(family, metric, d):
    return coherent(family, metric, d, N, np.random.default_rng(zlib.crc32(f"cpu/{family}/{metric}/{d}".encode())))


_WORST = {}


def worst(family, metric, d, rounding):
    key = (family, metric, d, rounding.__name__)
    if key not in _WORST:
        rows, q, _ = case(family, metric, d)
        _WORST[key] = float(model_ratios(metric, rows, q, rounding).max())
    return _WORST[key]


def test_the_roundings_on_known_bit_patterns():
    x = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F80C000, 0xBF808000, 0x3FFF8000, 0x00000000, 0x80000000],
                 dtype=np.uint32).view(np.float32)
    up = lambda f: (f(x).view(np.uint32) >> 16).tolist()
    assert up(bf16_rne) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0xBF80, 0x4000, 0x0000, 0x8000]
    assert up(bf16_half_up) == [0x3F81, 0x3F82, 0x3F80, 0x3F81, 0x3F81, 0xBF81, 0x4000, 0x0000, 0x8000]
    assert up(bf16_truncate) == [0x3F80, 0x3F81, 0x3F80, 0x3F80, 0x3F80, 0xBF80, 0x3FFF, 0x0000, 0x8000]
    for f in (bf16_rne, bf16_half_up, bf16_truncate):
        assert not (f(x).view(np.uint32) & 0xFFFF).any()


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_generators_deliver_the_stated_bits(family, d):
    low, parity = FAMILIES[family]
    for metric in METRICS:
        rows, q, pattern = case(family, metric, d)
        assert rows.shape == (N, d) and rows.dtype == np.float32 and q.shape == (COHERENT_QUERIES, d) and q.dtype == np.float32
        assert np.isfinite(rows).all() and np.isfinite(q).all() and (rows != 0).all()
        b = rows.view(np.uint32)
        assert ((b & 0xFFFF) == low).all()
        odd = (b >> 16) & 1
        if parity is None:
            assert 0.4 < odd.mean() < 0.6
        else:
            assert (odd == parity).all()
        expo = ((b >> 23) & 0xFF).astype(np.int64) - 127
        assert (expo == expo[:, :1]).all() and expo.min() >= -20 and expo.max() <= 20 and expo.min() < -10 and expo.max() > 10
        assert set(np.unique(pattern)) == {-1.0, 1.0}
        assert (rows[0::2] > 0).all() and (np.sign(rows[1::2]) == pattern).all()
        # the roundings on them: where they differ and where they cannot
        r, h = bf16_rne(rows), bf16_half_up(rows)
        if family in ("below", "above", "three_quarter", "tie_odd"):
            assert np.array_equal(r.view(np.uint32), h.view(np.uint32))
        elif family == "tie_even":
            assert (np.abs(h) > np.abs(r)).all()
        else:
            assert 0.4 < (np.abs(h) > np.abs(r)).mean() < 0.6
        assert (np.abs(h) >= np.abs(rows)).all() if low >= 0x8000 else (np.abs(h) < np.abs(rows)).all()
        # every element is a quarter ulp (three_quarter) or half an ulp off, to the last bit or one short of it
        ulp = np.exp2(expo - 7).astype(np.float64)
        off = np.abs(rows.astype(np.float64) - h.astype(np.float64)) / ulp
        assert np.allclose(off, 0.25 if family == "three_quarter" else 0.5, rtol=0, atol=2.0 ** -15)
        # the queries
        assert (q[0] == 1).all() and np.array_equal(q[1], pattern)
        for i in (0, 1, 2, 3):
            assert np.array_equal(bf16_rne(q[i]), q[i])
        assert np.array_equal(q[2], 3 * q[0]) and np.array_equal(q[3], 0.375 * q[1])
        assert ((q[4:6].view(np.uint32) & 0xFFFF) == 0x8000).all() and (np.sign(q[5]) == pattern).all()
        assert np.array_equal(q[6], 2 * rows[(N // 3) & ~1]) and np.array_equal(q[7], 0.25 * rows[(2 * N // 3) | 1])
        assert np.isfinite(np.linalg.norm(rows.astype(np.float32), axis=1) ** 2 * 4).all()      # Euclid's f32 squares stay finite


def test_tie_free_data_has_no_tie():
    rows, q = tie_free(192, 3000, 5, np.random.default_rng(5))
    assert ((rows.view(np.uint32) & 0xFFFF) != 0x8000).all()
    assert np.array_equal(bf16_rne(rows).view(np.uint32), bf16_half_up(rows).view(np.uint32))


def test_make_case_takes_a_dimension():
    rows, q = make_case("cancel", 2, np.random.default_rng(1), d=128)
    assert rows.shape == (66_000, 128) and q.shape == (48, 128)
    rows, q = make_case("cancel", 2, np.random.default_rng(1))
    assert rows.shape == (66_000, 96)


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_model_stays_inside_the_budget_under_both_roundings(family, metric, d):
    for rounding in (bf16_rne, bf16_half_up):
        assert worst(family, metric, d, rounding) <= 1.0, (rounding.__name__, worst(family, metric, d, rounding))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family", ["below", "above"])
def test_below_and_above_are_the_worst_case_of_both_roundings(family, metric):
    for rounding in (bf16_rne, bf16_half_up):
        assert worst(family, metric, 64, rounding) >= 0.9, (rounding.__name__, worst(family, metric, 64, rounding))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family", ["tie_even", "tie_odd", "tie_mixed"])
def test_every_tie_family_is_the_worst_case_of_half_up(family, metric):
    assert worst(family, metric, 64, bf16_half_up) >= 0.9, worst(family, metric, 64, bf16_half_up)


@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", METRICS)
def test_a_truncating_codec_breaks_the_budget_on_three_quarter(metric, d):
    """... so the GPU test over SPLIT rows would catch a layout codec that merely truncates."""
    assert worst("three_quarter", metric, d, bf16_truncate) > 1.0, worst("three_quarter", metric, d, bf16_truncate)

"""tests/split_schedule.py on the CPU: the numpy restatement of csrc/row_split.h, the schedule over the numpy store (every metric,
both rules, a screening floor of 1024 rows), and its three MUTANTS, each proved caught.  tests/test_gpu_split_paths.py runs the same
schedule over the engine.  No GPU needed."""
import numpy as np
import pytest

import split_schedule as ss

FLOOR = 1024


def rows_and_queries(metric, d):
    rng = np.random.default_rng([411, metric, d])
    rows = rng.standard_normal((FLOOR + 37, d)).astype(np.float32)
    bits = rows.view(np.uint32)
    bits[::7, 0] = (bits[::7, 0] & 0xffff0000) | 0x8000               # ties and full low halves, as the GPU data has them
    bits[::11, 1] |= 0xffff
    return rows, rng.standard_normal((9, d)).astype(np.float32)


def run(metric, d, mode, mutant=None):
    rows, q = rows_and_queries(metric, d)
    a = ss.SimIndex(metric, 0, rows, FLOOR)
    b = ss.SimIndex(metric, mode, rows, FLOOR, mutant=mutant)
    return ss.run_schedule(a, b, metric, mode, rows, q, floor=FLOOR)


def test_row_split_restated():
    """the codec of csrc/row_split.h in numpy: a bijection (sampled: every upper half with the low halves around the tie, and a
    million random patterns), zero stays zero, hi is the element rounded half up in magnitude"""
    rng = np.random.default_rng(5)
    upper = np.arange(1 << 16, dtype=np.uint32) << 16
    lows = np.array([0, 1, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.uint32)
    bits = np.concatenate([(upper[:, None] | lows[None, :]).ravel(), rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)])
    hi, lo = ss.split_hi(bits), ss.split_lo(bits)
    assert hi.dtype == lo.dtype == np.uint16 and np.array_equal(ss.split_join(hi, lo), bits)
    assert ss.split_hi(0) == 0 and ss.split_lo(0) == 0
    assert ss.split_hi(0x3f808000) == 0x3f81 and ss.split_hi(0x3f807fff) == 0x3f80 and ss.split_hi(0xbf808000) == 0xbf81
    assert ss.split_hi(0x7f7f8000) == 0x7f80 and not ss.split_nonfinite(0x7f7f8000)     # a finite element whose hi word is the bf16 infinity
    assert ss.split_nonfinite(np.array([0x7f800000, 0xff800000, 0x7fc00000, 0xffffffff], dtype=np.uint32)).all()
    finite = bits[~ss.split_nonfinite(bits)]
    x = finite.view(np.float32).astype(np.float64)
    h = (ss.split_hi(finite).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    ulp = np.maximum(np.abs(x), 2.0 ** -126) * 2.0 ** -7              # at least one bf16 ulp of x
    ok = np.isfinite(h)
    assert (np.abs(h[ok] - x[ok]) <= ulp[ok] / 2).all()              # within half an ulp wherever hi is finite ...
    assert (np.abs(x[~ok]) >= 3.3895e38).all()                       # ... and it is not only at the top of the range (0x7f7f8000 on)


@pytest.mark.parametrize("mode", [2, "adaptive"])
@pytest.mark.parametrize("metric,d", [(0, 64), (1, 40), (2, 64)])
def test_the_schedule_over_the_numpy_store(metric, d, mode):
    rule = run(metric, d, mode)
    assert rule.forward >= 6 and rule.back >= 6 and rule.refusals == 1 and rule.layout == ss.SPLIT


def test_the_numpy_store_keeps_its_rows_as_bytes():
    """what the mutants rest on: SPLIT bytes taken as floats are not the rows, joined they are, and an f32 row appended behind
    split rows does not survive the conversion back"""
    rows, q = rows_and_queries(0, 64)
    ix = ss.SimIndex(0, 2, rows, FLOOR)
    ix.search(q, 10)
    assert ix.layout() == (ss.SPLIT, 1)
    assert np.array_equal(ix._joined().view(np.uint32), rows.view(np.uint32))
    assert not np.array_equal(ix._as_floats().view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(ix.rows_f32().view(np.uint32), rows.view(np.uint32)) and ix.layout() == (ss.F32, 2)
    bad = ss.SimIndex(0, 2, rows, FLOOR, mutant="append_into_split")
    bad.search(q, 10)
    bad.add(10 ** 6, q[0])
    bad.search(q, 10)
    assert np.array_equal(bad._joined()[:len(rows)].view(np.uint32), rows.view(np.uint32))
    assert not np.array_equal(bad._joined()[-1].view(np.uint32), q[0].view(np.uint32))


# the step at which each mutant must show: (under mode 2, under the adaptive rule) -- a refusal is met by the first search under
# mode 2 and, the count starting again at every mutation, by the third search after the remove under the adaptive rule
CAUGHT_AT = {"reader_takes_bytes": ("by id over split rows",) * 2, "append_into_split": ("after add",) * 2,
             "refusal_forgotten": ("with the inf row", "tombstoned, still stored")}


@pytest.mark.parametrize("mode", [2, "adaptive"])
@pytest.mark.parametrize("mutant", ss.MUTANTS)
def test_every_mutant_is_caught(mutant, mode):
    assert set(CAUGHT_AT) == set(ss.MUTANTS)
    with pytest.raises(AssertionError) as e:
        run(0, 64, mode, mutant=mutant)
    assert CAUGHT_AT[mutant][mode != 2] in str(e.value), (mutant, mode, str(e.value)[:300])

"""The certificate (test_gpu_certificate.py) on the score paths that file cannot reach, and on the worst case of the bound.

  * SPLIT rows.  Every long-running index with ld % 64 == 0 ends up SPLIT, and the filter pass then reads the hi plane: each
    element rounded half up in magnitude, not to nearest even (row_split.h).  debug_screen_scores(split=True) dumps the scores
    of that pass over the store as it lies; checks (A), (B), (C) run on them, (C) with the rows rounded by bf16_half_up.
  * The 512-query kernel (kernels_fused_bf16w.hip): debug_screen_scores(wide=True) launches it as a search does; its scores
    must carry the bits of the 256-query passes.
  * COHERENT rounding errors (certificate_data.py): rows whose elements are all half a bf16 ulp off in the direction of their
    sign, queries proportional to that error.  test_certificate_cpu.py shows that exact arithmetic on the rounded operands
    uses 0.96 - 0.98 of the budget there; what the kernel's f32 accumulation and the oracle's f32 fold add must fit into the
    rest.  The condition is the certificate's own: zero (A) violations, ratios <= 1.0.

Shapes: 256 C + 77 rows on C compute units -- some workgroups run two tiles, the last tile is ragged -- and a few hundred
tombstones.  Worst ratios go to the margins file that test_gpu_certificate.py's fixture writes, keyed layout/kernel/...
"""
import ctypes
import zlib

import numpy as np
import pytest

from certificate_data import (COHERENT_QUERIES, FAMILIES, bf16_half_up, bf16_rne, coherent, exact_distances, make_case,
                              tie_free)
from test_gpu_certificate import MARGINS, bound_checks, vdb  # noqa: F401  (the fixture that writes the margins file)
from test_gpu_s16_tile_start import cu_count
from test_gpu_split_rows import F32, SPLIT, make_pair

pytestmark = pytest.mark.gpu

METRIC_NAMES = ["euclid", "cosine", "dot"]
ROUNDING = {"f32": bf16_rne, "split": bf16_half_up}      # what the filter pass reads a row in, by layout
FLAG_SPLIT, FLAG_WIDE = 4, 8                             # include/vdb_flat.h VDB_DEBUG_SCORES_*


def n_rows():
    return 256 * cu_count() + 77                         # (= 2 * 128 C + 77: the wide kernel's 128-row tiles, three for some workgroups)


def tombstones(n):
    """a few hundred: at the head, in the ragged tail, the last row of the first full tile"""
    return sorted(set(range(3, 900, 7)) | set(range(max(n - 400, 901), n, 3)) | {255})


def index(vdb, metric, rows, split_mode=None, dead=None):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    if split_mode is not None:
        ix.set_split(split_mode)
    ix.add_bulk(rows)
    live = np.ones(len(rows), dtype=bool)
    for r in tombstones(len(rows)) if dead is None else dead:
        ix.remove(r)
        live[r] = False
    return ix, live


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def shared_distances(metric, rows, q):
    """dist_of(b) for bound_checks: the oracle's distances of query b, computed once however many dumps are checked"""
    memo = {}

    def dist_of(b):
        if b not in memo:
            memo[b] = exact_distances(metric, rows, q[b])
        return memo[b]
    return dist_of


# ------------------------------------------------------------------ (a) the first file's kinds over SPLIT rows
@pytest.mark.parametrize("kind", ["cancel", "scales", "dim16384", "bf16ties", "subnormal"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_score_error_over_split_rows_stays_inside_the_certified_bound(vdb, metric, kind):
    """Checks (A), (B), (C) of test_gpu_certificate.py on the scores of the filter pass over SPLIT rows.  cancel runs at
    d = 128 (its own 96 cannot be SPLIT), dim16384 is the largest pitch a SPLIT store takes; 16 of a kind's queries, both
    halves of the kinds that have two sorts."""
    rng = np.random.default_rng(zlib.crc32(f"{metric}/{kind}".encode()))
    rows, q = make_case(kind, metric, rng, d=128 if kind == "cancel" else None)
    rows = np.ascontiguousarray(rows[:min(len(rows), n_rows())])
    q = np.ascontiguousarray(q[np.r_[0:8, len(q) - 8:len(q)]] if len(q) > 16 else q)
    ix, live = index(vdb, metric, rows, dead=[r for r in tombstones(len(rows)) if r >= 8])   # (rows 0..7 keep Cosine defined under "subnormal")
    assert ix.layout() == (F32, 0)
    bound_checks(ix, metric, kind, rows, q, f"split/fused_s16/{METRIC_NAMES[metric]}/{kind}", split=True, round_rows=bf16_half_up, live=live)
    assert ix.layout() == (SPLIT, 1)                     # after the dumps and after the probes
    ix.debug_row_info()
    ix.debug_cert_probe(np.zeros(4, np.uint32), np.zeros(4, np.float32), np.ones(4, np.float32))
    assert ix.layout() == (SPLIT, 1)


# ------------------------------------------------------------------ (b) the coherent families on both layouts
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_coherent_rounding_errors_stay_inside_the_bound_on_both_layouts(vdb, metric, family, d):
    """The worst case of the bound on F32 rows and on SPLIT rows of ONE index: (A), (B), and (C) with the layout's own
    rounding -- on tie_even over SPLIT rows the RNE operands are off by about K 2^-8 per unit of |q||d|, far outside c_acc, so
    (C) passes only if the kernel read hi at every k offset and pitch.  Where the two roundings agree on every element the
    two layouts' scores agree bit for bit; on tie_even they differ, and (Dot) equal those of an F32 index that stores
    bf16_half_up(rows).  The store goes F32 -> SPLIT -> F32 whatever set_split says, and comes back bit for bit."""
    rng = np.random.default_rng(zlib.crc32(f"coherent/{family}/{metric}/{d}".encode()))
    n = n_rows()
    rows, q, _ = coherent(family, metric, d, n, rng)
    ix, live = index(vdb, metric, rows, split_mode=metric)   # never / adaptive / before the next search: the dump ignores all three
    dist_of = shared_distances(metric, rows, q)
    got = {}
    for layout in ("f32", "split"):
        key = f"{layout}/{'fused_s16' if layout == 'split' else 'fused_bf16p'}/{METRIC_NAMES[metric]}/{family}/d{d}"
        got[layout] = bound_checks(ix, metric, family, rows, q, key, split=layout == "split", round_rows=ROUNDING[layout],
                                   dist_of=dist_of, live=live)
        assert MARGINS[key]["queries_outside_the_certifiable_domain"] == 0
        assert ix.layout() == ((F32, 0) if layout == "f32" else (SPLIT, 1))
    back = (ix.debug_screen_scores(q, raw=1)[0], ix.debug_screen_scores(q, raw=0)[0])
    assert ix.layout() == (F32, 2)
    for a, b in zip(got["f32"], back):
        assert np.array_equal(bits(a), bits(b)), "the rows did not come back from SPLIT bit for bit"
    for raw, (a, b) in enumerate(zip(got["f32"][::-1], got["split"][::-1])):
        if family in ("below", "above", "three_quarter", "tie_odd"):
            assert np.array_equal(bits(a), bits(b)), (family, raw, "no element is rounded differently, yet the scores differ")
        elif family == "tie_even":
            assert not np.array_equal(bits(a), bits(b)), (family, raw, "every element is rounded differently, yet no score differs")
    if family == "tie_even" and metric == 2:
        hx, _ = index(vdb, metric, bf16_half_up(rows), split_mode=0)
        want = hx.debug_screen_scores(q, raw=1)[0]
        assert hx.layout() == (F32, 0)
        assert np.array_equal(bits(want), bits(got["split"][0])), "SPLIT scores are not those of the hi plane"


# ------------------------------------------------------------------ (c) no tie element: the layouts agree on every bit
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_split_scores_equal_f32_scores_without_tie_elements(vdb, metric, d):
    rows, q = tie_free(d, n_rows(), 256, np.random.default_rng(31 * d + metric))
    ix, live = index(vdb, metric, rows)
    cases = [(nq, raw) for nq in (1, 19, 256) for raw in (0, 1)]
    plain = {c: ix.debug_screen_scores(q[:c[0]], raw=c[1])[0] for c in cases}
    assert ix.layout() == (F32, 0)
    for nq, raw in cases:
        s = ix.debug_screen_scores(q[:nq], raw=raw, split=True)[0]
        assert s.shape == (nq, len(rows))
        assert np.array_equal(bits(s), bits(plain[(nq, raw)])), (metric, d, nq, raw)
        assert np.isfinite(s[:, live]).all() and np.isnan(s[:, ~live]).all()
    assert ix.layout() == (SPLIT, 1)


# ------------------------------------------------------------------ (d) the thresholds of a search do not depend on the layout
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_thresholds_agree_between_the_layouts(vdb, metric, d):
    """The sample pass reads an RNE copy of its rows in both layouts, so the filter thresholds of the same search agree bit
    for bit -- also on rows made of tie elements alone (gaussian values, low halves forced to 0x8000 under even upper halves),
    where every score of the filter pass itself differs between the layouts."""
    rng = np.random.default_rng(900 + 3 * d + metric)
    rows = rng.standard_normal((n_rows(), d), dtype=np.float32) * rng.uniform(0.1, 4.0, (n_rows(), 1)).astype(np.float32)
    rows = ((rows.view(np.uint32) & np.uint32(0xFFFE0000)) | np.uint32(0x8000)).view(np.float32)
    q = rng.standard_normal((19, d), dtype=np.float32)
    a, b = make_pair(vdb, metric, rows)
    ra, rb = a.search_batch_arrays(q, 10), b.search_batch_arrays(q, 10)
    ta, tb = a.debug_last_thresholds(len(q)), b.debug_last_thresholds(len(q))
    for ix in (a, b):                                    # the screening tier answered alone: these are its thresholds
        st = ix.last_stats()
        assert st["bf16_screen"] == 1 and st["f32_tier_queries"] == 0 and st["exact_queries"] == 0, st
    assert a.layout() == (F32, 0) and b.layout() == (SPLIT, 1)
    assert np.isfinite(ta).all() and np.array_equal(bits(ta), bits(tb)), (ta, tb)
    for x, y in zip(ra, rb):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    sa, sb = a.debug_screen_scores(q, raw=1)[0], b.debug_screen_scores(q, raw=1, split=True)[0]
    assert not np.array_equal(bits(sa), bits(sb))        # ... while the filter pass did read another rounding of the rows


# ------------------------------------------------------------------ (e) the wide kernel
@pytest.mark.parametrize("d", [64, 192])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_wide_kernel_scores_equal_the_256_query_passes_bit_for_bit(vdb, metric, d):
    rows, q = tie_free(d, n_rows(), 512, np.random.default_rng(77 * d + metric))
    ix, live = index(vdb, metric, rows)
    for nq in (257, 300, 512):
        for raw in (0, 1):
            w = ix.debug_screen_scores(q[:nq], raw=raw, wide=True)[0]
            two = np.concatenate([ix.debug_screen_scores(q[:256], raw=raw)[0], ix.debug_screen_scores(q[256:nq], raw=raw)[0]])
            assert w.shape == (nq, len(rows))
            assert np.array_equal(bits(w), bits(two)), (metric, d, nq, raw)
            assert (bits(w)[:, ~live] == 0xFFFFFFFF).all() and not (bits(w)[:, live] == 0xFFFFFFFF).any()
    assert ix.layout() == (F32, 0)


@pytest.mark.parametrize("metric", [2, 1])
def test_wide_kernel_stays_inside_the_bound_on_coherent_rows(vdb, metric):
    """(A) and (B) (and under Dot (C)) through the 512-query kernel, on family below at d = 64: the 16 coherent queries 17
    times over make a batch the wide kernel serves (272 queries, both 256-query blocks in use)."""
    rows, q16, _ = coherent("below", metric, 64, n_rows(), np.random.default_rng(4100 + metric))
    q = np.ascontiguousarray(np.tile(q16, (17, 1)))
    ix, live = index(vdb, metric, rows)
    d16 = shared_distances(metric, rows, q16)
    bound_checks(ix, metric, "below", rows, q, f"f32/fused_bf16w/{METRIC_NAMES[metric]}/below/d64", wide=True,
                 dist_of=lambda b: d16(b % COHERENT_QUERIES), live=live)
    assert ix.layout() == (F32, 0)


# ------------------------------------------------------------------ (f) what the dump refuses
def dump_rc(vdb, ix, q, flags):
    """the C call's own return code (the Python wrapper raises one exception type for several codes)"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    scores = np.zeros((q.shape[0], int(ix._L.vdb_flat_debug_rows(ix._h))), dtype=np.float32)
    return ix._L.vdb_flat_debug_screen_scores(ix._h, q.ctypes.data_as(fp), q.shape[0], q.shape[1], int(flags),
                                              scores.ctypes.data_as(fp), None, None)


def test_the_dump_refuses_what_no_search_would_run(vdb):
    INVALID = vdb._ffi.ERR_INVALID_ARGUMENT
    rng = np.random.default_rng(12)
    n = 3000
    rows, q = tie_free(64, n, 300, rng)

    def refused(ix, q, flags, before):
        assert dump_rc(vdb, ix, q, flags) == INVALID, flags
        assert vdb._ffi.last_error()[0], "a refusal names its reason"
        assert ix.layout() == before, flags

    ix, _ = index(vdb, 2, rows)
    ix.set_shadow(True)
    refused(ix, q[:5], FLAG_SPLIT, (F32, 0))                                   # the filter pass would read the shadow
    ix.set_shadow(False)
    for flags in (FLAG_SPLIT | 2, FLAG_SPLIT | FLAG_WIDE, FLAG_SPLIT | FLAG_WIDE | 1):
        refused(ix, q, flags, (F32, 0))
    refused(ix, q[:256], FLAG_WIDE, (F32, 0))                                  # no search runs the wide kernel on 256 queries
    refused(ix, q[:256], FLAG_WIDE | 1, (F32, 0))
    refused(ix, q, FLAG_WIDE | 2, (F32, 0))
    assert dump_rc(vdb, ix, q[:5], FLAG_SPLIT) == 0 and ix.layout() == (SPLIT, 1)
    for flags in (FLAG_SPLIT | 2, FLAG_SPLIT | FLAG_WIDE):                     # ... and a SPLIT store stays SPLIT through a refusal
        refused(ix, q, flags, (SPLIT, 1))
    with pytest.raises(vdb.IndexError_):
        ix.debug_screen_scores(q, raw=2, split=True)
    with pytest.raises(vdb.IndexError_):
        ix.debug_screen_scores(q[:256], wide=True)

    ix96, _ = index(vdb, 2, rng.standard_normal((n, 96), dtype=np.float32))    # ld = 96: no SPLIT layout
    refused(ix96, rng.standard_normal((5, 96), dtype=np.float32), FLAG_SPLIT, (F32, 0))

    bad = rows.copy()
    bad[n // 2, 3] = np.inf
    ixb, _ = index(vdb, 2, bad)
    refused(ixb, q[:5], FLAG_SPLIT, (F32, 2))                                  # forward, found out, straight back
    refused(ixb, q[:5], FLAG_SPLIT | 1, (F32, 2))                              # and not tried again while the rows stay
    assert dump_rc(vdb, ixb, q[:5], 1) == 0 and ixb.layout() == (F32, 2)       # the plain dump still serves it

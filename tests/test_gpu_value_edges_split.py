"""The value families of tests/value_families.py over SPLIT rows: every (family, metric) at the screening tier's
row floor and at the large-k shape under set_split(2), with the suite's tombstones and its 50 % mask, the hidden row tombstoned
and alive.  tests/test_gpu_value_edges.py runs the same families over f32 rows; here the filter pass reads the hi plane and the
re-ranks join every element from its two halves.

Results are compared with the oracle on ids, counts and distance BITS, or with the oracle's error (same class, one message on
every route), exactly as tests/test_gpu_value_edges.py does.  No tolerance anywhere.

The layout after every search is predicted, not observed:
  * a store that holds ANY non-finite element -- in a tombstoned row too: the conversion walks the rows, not the live bits -- is
    converted forward, found out, converted straight back and not tried again: (F32, 2) from the first search on (inf_tail, and
    nan_hidden whether its row is hidden or not);
  * a live zero-norm row under Cosine fails the search before any tier runs: (F32, 0);
  * every other store is converted forward by its first search.  It is SPLIT afterwards unless that search handed a query to the
    f32 tier or to the exact scan, which read f32 rows (the hand-over inside search_part2 converts back, once).  Which family
    does is written down below (HANDS_OVER, with the reason from the certificate) and asserted search by search: the counters of
    last_stats() against the table, the layout against the table -- never the layout against the counters."""
import numpy as np
import pytest

import value_families as vf
from conftest import load_package
from test_gpu_value_edges import check_oracle, expect_error, same

pytestmark = pytest.mark.gpu

F32, SPLIT = 0, 1
# The re-rank certifies a query when its k-th exact distance, widened by the error bound of the bf16 scores (proportional to
# |q| |d|, plus the per-row margins), still lies below the score of the first candidate it did not re-rank.  That cannot hold
#   * across a tie group wider than the candidate depth: the first candidate left out scores what the k-th does;
#   * beside a norm that is infinite: the bound is.
# Every family but the gaussian ones is built on one of the two, at every metric, shape and mask of this module, for at least one
# query of every batch -- so each of their searches converts forward (mode 2) and back: two conversions, F32 afterwards.
HANDS_OVER = {
    "overflow": "query 0 overflows its own norm (|q| = inf), and the rows whose squares overflow have infinite norms",
    "bf16_edge": "FLT_MAX squared overflows: the special rows have infinite norms, and under Dot and Cosine they ARE the top-k",
    "subnormal": "tie groups of half the index (Euclid, the gaussian queries) and products that underflow to one value (the tiny queries)",
    "cos_den_tiny": "norms at the bottom of f32: the scores of the tiny rows fall inside the bound, duplicates among them",
    "cos_den_clamp": "every row is a multiple of one direction: a handful of distinct distances, tie groups of thousands of rows",
    "dot_zero": "a -0.0 tie group of 60 % of the rows",
}
NEVER_HAND_OVER = {"tame", "cos_den_zero"}                          # gaussian rows (the zero-norm row hidden): certified on the screening tier
REFUSED = {"inf_tail", "nan_hidden"}                                # a non-finite element in the store: F32 whatever the tiers do
assert set(HANDS_OVER) | NEVER_HAND_OVER | REFUSED == set(vf.FAMILIES)


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def shape_of(vdb, name):
    if name == "large_k":
        return vf.large_k_split_shape(vdb._ffi.lib().vdb_flat_large_k_min_rows(vf.K_LARGE))     # d = 64: a pitch the layout takes
    return vf.SHAPES[name]


def build(vdb, family, metric, n, d, nq, hide):
    rows, q = vf.make(family, n, d, nq, metric)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    ix.set_split(2)
    ix.add_bulk(rows)
    for r in vf.dead_rows(n, hide):
        ix.remove(int(r))
    return ix, rows, q


class Layout:
    """the prediction of the module docstring, advanced search by search"""

    def __init__(self, family, rows):
        self.refused = not np.isfinite(rows).all()
        assert self.refused == (family in REFUSED)
        self.hands_over = family in HANDS_OVER
        self.layout, self.conv = F32, 0

    def search(self, failed_before_the_tiers=False):
        if failed_before_the_tiers:
            return
        if self.refused:
            if self.conv == 0:
                self.conv = 2                                       # forward, found out, back; never again
            return
        if self.layout == F32:
            self.layout, self.conv = SPLIT, self.conv + 1           # mode 2: before every eligible search
        if self.hands_over:
            self.layout, self.conv = F32, self.conv + 1             # the hand-over inside the search

    def expect(self):
        return self.layout, self.conv


@pytest.mark.parametrize("shape", ["screened", "large_k"])
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_families_over_split_rows(vdb, family, metric, shape):
    n, d, nq, (k,) = shape_of(vdb, shape)
    error = vf.FAMILIES[family][2]
    for hide in (True, False):
        ix, rows, q = build(vdb, family, metric, n, d, nq, hide)
        lay = Layout(family, rows)
        live = vf.live_bytes(n, hide)
        on, words = vf.id_mask(n, 0.5, 7, hide=hide)
        tag = "%s-hide%d" % (shape, hide)
        what = (family, metric, shape, hide)

        def step(name, st, **kw):
            lay.search(**kw)
            print(what, name, "predicted", lay.expect(), "seen", ix.layout(), st)
            assert ix.layout() == lay.expect(), what + (name, "predicted", lay.expect(), "seen", ix.layout(), st)
            if st is not None:
                assert st["bf16_screen"] == 1, what + (name, st)
                if family in NEVER_HAND_OVER:
                    assert st["mfma_queries"] == nq and st["f32_tier_queries"] == 0 and st["exact_queries"] == 0, what + (name, st)
                if family in HANDS_OVER:
                    assert st["f32_tier_queries"] + st["exact_queries"] > 0 and st["mfma_queries"] < nq, what + (name, HANDS_OVER[family], st)
                if (family, metric) == ("subnormal", vf.DOT):       # exactly the tiny (even) queries
                    assert st["f32_tier_queries"] == st["exact_queries"] == nq // 2 and st["mfma_queries"] == nq // 2, what + (name, st)

        if error and not hide:
            # the oracle errors while the row is alive and eligible: plain, and under the mask that admits it
            zero_norm = error == "InvalidVector"
            msg = expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k))
            step("plain error", None, failed_before_the_tiers=zero_norm)
            expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k, id_mask=words, mask_bits=n), msg)
            step("masked error", None, failed_before_the_tiers=zero_norm)
            # under the mask that excludes it a NaN row is never computed; a zero-norm row under Cosine still fails the call
            off, off_words = vf.id_mask(n, 0.5, 7, hide=True)
            if zero_norm:
                expect_error(vdb, family, lambda: ix.search_batch_arrays(q, k, id_mask=off_words, mask_bits=n), msg)
                step("excluded, still an error", None, failed_before_the_tiers=True)
            else:
                res = ix.search_batch_arrays(q, k, id_mask=off_words, mask_bits=n)
                step("excluded", ix.last_stats())
                check_oracle(res, family, metric, n, d, nq, k, live & off, tag=tag + "-off")
            continue
        res = ix.search_batch_arrays(q, k)
        st = ix.last_stats()
        step("plain", st)
        check_oracle(res, family, metric, n, d, nq, k, live, tag=tag, what=st)
        again = ix.search_batch_arrays(q, k)                        # once more, from whatever layout the first search left
        step("plain again", ix.last_stats())
        assert same(res, again), what
        masked = ix.search_batch_arrays(q, k, id_mask=words, mask_bits=n)
        st = ix.last_stats()
        step("half mask", st)
        check_oracle(masked, family, metric, n, d, nq, k, live & on, tag=tag + "-half", what=st)
        if shape == "large_k":                                      # every query through the re-threshold pass as well
            ix.set_tiers(ix.TIERS_FORCE_RETHRESHOLD)
            try:
                other = ix.search_batch_arrays(q, k)
                st = ix.last_stats()
            finally:
                ix.set_tiers(0)
            step("forced re-threshold", st)
            assert same(res, other), what + (st,)

"""The SPLIT row layout on every kernel and route that reads the rows: ragged dimensions, the large-k re-rank and
the re-threshold pass, masks and tombstones, batches of several passes, every composed read, two tickets in flight, a non-finite
element that arrives late, every mutation under both conversion rules (the schedule of tests/split_schedule.py), the sharded
handle.  tests/test_gpu_split_rows.py holds the layout's basics at d = 64 / 192 / 768.

A reader that forgets rows_f32() raises nothing: it reads permuted halves as floats and returns plausible wrong neighbours.  So
every comparison is bit for bit (ids, counts, distance bits; score bits for MMR) between an index that never converts (mode 0) and
one that does (mode 2, or the adaptive rule with a run of RUN searches), and against the CPU oracle or the contract models of the
read (by_id_data, recommend_data, mmr_data, distinct_data, per_group_data, range_data).  No tolerance anywhere.

Every test asserts the route it means to take (layout(), last_stats(), the read's own counters).  Where a test predicts the layout
after a call and the number of conversions the call made, the prediction is derived beside the case from the rule of DESIGN 4.3:
  * a screened search of at most 256 queries over a split-able store (ld % 64 == 0, no shadow) is ELIGIBLE: under mode 2 it
    converts forward first; under the adaptive rule it converts first when RUN eligible searches were counted, then counts itself;
  * rows_f32() -- every reader other than the filter pass and the four re-ranks -- converts back and resets the count;
  * rows_mut() -- every mutation of the rows -- does the same and forgets a refusal;
  * a change of the sample size S between two searches (k <= 58 and k > 58 at 65 573 rows) rebuilds the compact sample copy from
    f32 rows: back, then forward again under mode 2.  The composed reads below keep to depths of at most 58 (or, at the large
    shape, to one S for every depth) so that this does not enter their predictions."""
import numpy as np
import pytest

import oracle
import by_id_data as bd
import distinct_data as dd
import mmr_data as md
import range_data as rgd
import recommend_data as rd
import value_families as vf
from conftest import load_package
from split_schedule import RUN, check_oracle, run_schedule, same         # RUN: the adaptive rule's run in these tests (debug_set_split_after)

pytestmark = pytest.mark.gpu

N = 65536 + 37                                     # the screening tier's minimum and a ragged last tile
F32, SPLIT = 0, 1
METRICS = (0, 1, 2)
U64 = np.uint64

_DATA, _IX, _MEMO = {}, {}, {}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    yield v
    _IX.clear()
    _DATA.clear()
    _MEMO.clear()


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def data(d, n=N, nq=40):
    """gaussian rows and queries of dimension d, made once and never written to.  Every 7th row has a tie in column 0, every
    11th a full low half in column 1: the two ends of what the low plane can hold."""
    if (n, d) not in _DATA:
        rng = np.random.default_rng([2031, n, d])
        rows = rng.standard_normal((n, d)).astype(np.float32)
        bits = rows.view(np.uint32)
        bits[::7, 0] = (bits[::7, 0] & 0xffff0000) | 0x8000
        bits[::11, 1] |= 0xffff
        q = rng.standard_normal((nq, d)).astype(np.float32)
        rows.setflags(write=False)
        q.setflags(write=False)
        _DATA[(n, d)] = rows, q
    return _DATA[(n, d)]


def new_index(vdb, metric, rows, mode, ids=None, **ctor):
    """mode 0 / 2, or "adaptive": mode 1 with a run of RUN"""
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **ctor)
    ix.add_bulk(rows, ids=ids)
    if mode == "adaptive":
        ix.set_split(1)
        ix.debug_set_split_after(RUN)
    else:
        ix.set_split(mode)
    return ix


def pair(vdb, metric, d, n=N, mode=2, keep=True):
    """(the mode-0 twin, the converting index) over data(d, n)"""
    key = (metric, n, d, mode)
    if key in _IX:
        return _IX[key]
    rows = data(d, n)[0]
    p = (new_index(vdb, metric, rows, 0), new_index(vdb, metric, rows, mode))
    if keep:
        _IX[key] = p
    return p


def to_split(ix, q, k=10):
    """eligible searches until the rows are SPLIT: one under mode 2, RUN + 1 under the adaptive rule"""
    for _ in range(RUN + 1):
        if ix.layout()[0] == SPLIT:
            break
        ix.search_batch_arrays(q[:2], k)
    assert ix.layout()[0] == SPLIT, ix.layout()


def to_f32(ix, some_id=9):
    """one f32 reader: the rows are F32 and the adaptive count is 0"""
    ix.get_vector(some_id)
    assert ix.layout()[0] == F32


def mask_words(on):
    m = np.packbits(np.asarray(on, dtype=np.uint8), bitorder="little")
    return np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64)


# ================================================================== a. ragged dimensions
# d = 33, 47, 100, 121, 750: ld = 64, 64, 128, 128, 768, all multiples of 64, tails of 1, 15, 4, 9 and 14 elements behind the last
# whole K slice.  d = 121: the padded dimension is 124 and the last slice is 4 mod 8 words long; d = 750: several slices a round.
RAGGED = (33, 47, 100, 121, 750)


@pytest.mark.parametrize("B,k", [(1, 1), (37, 10), (37, 100)])
@pytest.mark.parametrize("d", RAGGED)
@pytest.mark.parametrize("metric", METRICS)
def test_ragged_dimensions(vdb, metric, d, B, k):
    rows, queries = data(d)
    q = queries[:B]
    a, b = pair(vdb, metric, d)
    ra, sa = a.search_batch_arrays(q, k), a.last_stats()
    rb, sb = b.search_batch_arrays(q, k), b.last_stats()
    assert a.layout() == (F32, 0) and b.layout()[0] == SPLIT, (a.layout(), b.layout())
    assert sa["bf16_screen"] == 1 and sb["bf16_screen"] == 1, (sa, sb)
    assert same(ra, rb), (metric, d, B, k, sb)
    check_oracle(metric, rows, q, k, rb, sorted({0, B - 1}))


@pytest.mark.parametrize("d", [33, 750])
def test_ragged_rows_come_back_bit_for_bit(vdb, d):
    """forward, then get_vector: the original bits, d of them, for row 0, the rows of the last (partial) conversion batch, row
    N - 1 and two hundred others; then forward again and the search still equals the twin (a padding column that picked up a
    half of its neighbour would show in every dot product)"""
    rows, queries = data(d)
    ld = (d + 31) // 32 * 32
    per_batch = 16384 // ld
    tail = N % per_batch
    assert ld % 64 == 0 and 0 < tail < per_batch
    a, b = pair(vdb, 0, d)
    to_split(b, queries)
    c0 = b.layout()[1]
    sel = np.unique(np.concatenate([[0, 1, per_batch - 1, per_batch], np.arange(N - tail - 2, N),
                                    np.random.default_rng(d).integers(0, N, 200)]))
    for r in sel:
        v = np.asarray(b.get_vector(int(r)).as_slice(), dtype=np.float32)
        assert v.shape == (d,) and np.array_equal(v.view(np.uint32), rows[r].view(np.uint32)), (d, int(r))
        assert b.layout() == (F32, c0 + 1)                          # the first read converted back, the others find f32 rows
    rb = b.search_batch_arrays(queries[:5], 10)
    assert b.layout() == (SPLIT, c0 + 2) and same(a.search_batch_arrays(queries[:5], 10), rb)


@pytest.mark.parametrize("d", [65, 130])
def test_a_pitch_that_is_no_multiple_of_64_stays_f32(vdb, d):
    """ld = 96 and 160: the shadow-row kernel cannot run at the store's pitch, mode 2 changes nothing"""
    rows, queries = data(d)
    a, b = pair(vdb, 0, d, keep=False)
    for k in (10, 100):
        ra, rb = a.search_batch_arrays(queries[:37], k), b.search_batch_arrays(queries[:37], k)
        assert b.last_stats()["bf16_screen"] == 1 and b.layout() == (F32, 0)
        assert same(ra, rb)
    check_oracle(0, rows, queries, 100, rb, [0, 36])


# ================================================================== b. large k and the re-threshold pass over SPLIT rows
def large_n(vdb, k):
    return max(int(vdb._ffi.lib().vdb_flat_large_k_min_rows(k)), 65536) + 37


def run_large_k(vdb, metric, k, d, nq=9):
    n = large_n(vdb, k)
    rows, queries = data(d, n)
    q = queries[:nq]
    a, b = pair(vdb, metric, d, n)
    ra, sa = a.search_batch_arrays(q, k), a.last_stats()
    rb, sb = b.search_batch_arrays(q, k), b.last_stats()
    assert b.layout()[0] == SPLIT and a.layout() == (F32, 0)
    # gaussian rows: the large-k re-rank (rerank_large_kernel) certifies every query on both sides
    assert sa["bf16_screen"] == 1 and sb["bf16_screen"] == 1 and sb["kprime"] > 512, (sa, sb)
    assert sb["mfma_queries"] == nq and sb["exact_queries"] == 0 and sb["f32_tier_queries"] == 0, sb
    assert same(ra, rb), (metric, k, d, sb)
    check_oracle(metric, rows, q, k, rb, [0, nq - 1])
    return a, b, q, ra


@pytest.mark.parametrize("k,d", [(113, 64), (113, 40), (300, 64)])
@pytest.mark.parametrize("metric", METRICS)
def test_large_k_over_split_rows(vdb, metric, k, d):
    a, b, q, ra = run_large_k(vdb, metric, k, d)
    if k == 113:
        # every query through the re-threshold pass as well: rerank_all_large_kernel over SPLIT rows
        c0 = b.layout()[1]
        b.set_tiers(b.TIERS_FORCE_RETHRESHOLD)
        try:
            rb = b.search_batch_arrays(q, k)
            st = b.last_stats()
        finally:
            b.set_tiers(0)
        assert st["rethreshold_queries"] == len(q) and st["exact_queries"] == 0 and st["f32_tier_queries"] == 0, st
        assert b.layout() == (SPLIT, c0) and same(ra, rb)


def test_k_1024_over_split_rows(vdb):
    """one case of about 292 000 rows (the row floor of k = 1024): the deepest re-rank, Euclid only"""
    run_large_k(vdb, 0, 1024, 64, nq=3)
    _IX.pop((0, large_n(vdb, 1024), 64, 2))


@pytest.mark.parametrize("metric", METRICS)
def test_forced_tiers_at_small_k(vdb, metric):
    d, k = 64, 10
    rows, queries = data(d)
    q = queries[:9]
    a, b = pair(vdb, metric, d)
    ra = a.search_batch_arrays(q, k)
    to_split(b, queries)
    c0 = b.layout()[1]
    # the re-threshold pass (rerank_all_kernel) reads SPLIT rows as they lie
    b.set_tiers(b.TIERS_FORCE_RETHRESHOLD)
    try:
        rb, st = b.search_batch_arrays(q, k), b.last_stats()
    finally:
        b.set_tiers(0)
    assert st["rethreshold_queries"] == len(q) and st["exact_queries"] == 0, st
    assert b.layout() == (SPLIT, c0) and same(ra, rb)
    # the f32 tier reads f32 rows: the hand-over inside search_part2 converts back, once
    b.set_tiers(b.TIERS_FORCE_F32)
    try:
        rb, st = b.search_batch_arrays(q, k), b.last_stats()
    finally:
        b.set_tiers(0)
    assert st["bf16_screen"] == 1 and st["f32_tier_queries"] == len(q), st
    assert b.layout() == (F32, c0 + 1) and same(ra, rb)
    rb = b.search_batch_arrays(q, k)                               # mode 2: the next plain search converts forward again
    assert b.layout() == (SPLIT, c0 + 2) and same(ra, rb)
    check_oracle(metric, rows, q, k, rb, [0, 8])


# ================================================================== c. masks and tombstones with the sparse filter off
@pytest.mark.parametrize("metric", METRICS)
def test_masks_and_tombstones_over_split_rows(vdb, metric):
    d, k = 64, 10
    rows, queries = data(d)
    q = queries[:9]
    a, b = (new_index(vdb, metric, rows, m) for m in (0, 2))
    to_split(b, queries)
    c0 = b.layout()[1]
    live = np.ones(N, dtype=np.uint8)

    def both(what, **kw):
        ra, rb = a.search_batch_arrays(q, k, **kw), b.search_batch_arrays(q, k, **kw)
        st = b.last_stats()
        print(what, metric, b.layout(), st)
        assert st["bf16_screen"] == 1, (what, st)
        assert same(ra, rb), (what, st)
        return rb, st

    for sel in (0.5, 0.02):
        on = vf.id_mask(N, sel, 7, hide=False)[0]
        rb, st = both("mask %g" % sel, id_mask=mask_words(on), mask_bits=N)
        check_oracle(metric, rows, q, k, rb, [0, 8], live=on.astype(np.uint8))
        assert b.layout() == (SPLIT, c0), (sel, b.layout(), st)
    on = vf.short_mask(N)[0]
    rb, st = both("short mask", id_mask=mask_words(on), mask_bits=N)
    assert (rb[2] == 6).all()
    check_oracle(metric, rows, q, k, rb, [0, 8], live=on.astype(np.uint8))
    assert b.layout() == (SPLIT, c0), (b.layout(), st)
    # a compiled mask: code != 1 on a code column
    codes = (np.arange(N) % 3).astype(np.int32)
    t = vdb.MetaTable(0)
    try:
        t.set_codes(0, 0, codes)
        t.set_present(0, N, True)
        with t.compile([(vdb.MetaTable.NE, 0, 1)], N) as cm:
            assert cm.count() == int((codes != 1).sum())
            rb, st = both("compiled", compiled_mask=cm)
        check_oracle(metric, rows, q, k, rb, [0, 8], live=(codes != 1).astype(np.uint8))
        assert b.layout() == (SPLIT, c0), (b.layout(), st)
    finally:
        t.close()
    # tombstones without compaction.  remove() touches the live bitmask alone (kill_row): it does not ask for the rows
    dead = np.unique(np.concatenate([np.arange(0, 64), np.random.default_rng(5).integers(0, N, 300),
                                     oracle.flat_search(metric, rows, q[0], 3)[0].astype(np.int64)]))
    for ix in (a, b):
        for r in dead:
            ix.remove(int(r))
    assert b.layout() == (SPLIT, c0)
    live[dead] = 0
    rb, st = both("tombstones")
    check_oracle(metric, rows, q, k, rb, [0, 8], live=live)
    assert b.layout() == (SPLIT, c0), (b.layout(), st)
    on = vf.id_mask(N, 0.02, 7, hide=False)[0]
    rb, st = both("tombstones and mask", id_mask=mask_words(on), mask_bits=N)
    check_oracle(metric, rows, q, k, rb, [0, 8], live=live & on)
    assert b.layout() == (SPLIT, c0), (b.layout(), st)
    # the sparse route scans the eligible rows as f32 rows: back
    for ix in (a, b):
        ix.set_sparse_filter(1)
    ra = a.search_batch_arrays(q, k, id_mask=mask_words(on), mask_bits=N)
    rs = b.search_batch_arrays(q, k, id_mask=mask_words(on), mask_bits=N)
    assert b.sparse_stats()[0] == 1 and b.layout() == (F32, c0 + 1)
    assert same(ra, rs) and same(rb, rs)


# ================================================================== d. batches of several passes
@pytest.mark.parametrize("metric", METRICS)
def test_batches_above_256_queries(vdb, metric):
    """On a SPLIT index a batch above 256 queries runs as 256-query passes of the 4-wave kernel (the wide kernel reads f32
    rows), alternating between the two workspaces; with more than two passes all thresholds are computed first.  Such a batch
    neither counts nor converts."""
    d, k = 64, 10
    rows = data(d)[0]
    queries = memo("batch queries", lambda: np.random.default_rng(77).standard_normal((1024, d)).astype(np.float32))
    a, b = pair(vdb, metric, d)
    to_f32(b)
    c0 = b.layout()[1]
    ra = a.search_batch_arrays(queries, k)
    sa = a.last_stats()
    rb = b.search_batch_arrays(queries, k)                          # F32 rows, mode 2, 1024 queries: not eligible, no conversion
    sb = b.last_stats()
    assert b.layout() == (F32, c0) and same(ra, rb)
    assert sa["bf16_screen"] == 1 and sb["bf16_screen"] == 1 and sa["rethreshold_queries"] == 0, (sa, sb)
    assert sa["rows_scanned"] == 2 * N and sb["rows_scanned"] == 2 * N, (sa, sb)     # the wide kernel: two fetches of the rows
    check_oracle(metric, rows, queries, k, rb, [0, 255, 256, 1023])
    to_split(b, queries)
    c1 = b.layout()[1]
    for B in (512, 1024):
        for wide in (True, False):
            b.set_wide(wide)
            try:
                rb = b.search_batch_arrays(queries[:B], k)
                sb = b.last_stats()
            finally:
                b.set_wide(True)
            assert b.layout() == (SPLIT, c1), (B, wide, b.layout())
            assert sb["bf16_screen"] == 1 and sb["rethreshold_queries"] == 0 and sb["rows_scanned"] == (B // 256) * N, (B, wide, sb)
            assert same(tuple(x[:B] for x in ra), rb), (metric, B, wide, sb)


# ================================================================== e. every composed read
# One index per (metric, mode), every read once from SPLIT rows and once from F32 rows (just after an f32 reader: the adaptive count
# is 0).  A read is (call, model check, prediction): call(ix, metric) returns the arrays compared with the mode-0 twin and the number
# of eligible searches the call made (from the read's own counters where it varies); predict(mode, start, searches) returns
# (layout afterwards, conversions the call made).
D_E, K_E = 64, 10
NQ_E = 3


def _after_searches(mode, start, n_searches, reader_first=False, reader_last=False):
    """The rule of DESIGN 4.3 for a call made of an optional f32 reader, n eligible searches, an optional f32 reader."""
    layout, conv, streak = start, 0, (1 if start == SPLIT else 0)   # (after to_split the count is at least 1; it only matters from F32)
    if reader_first and layout == SPLIT:
        layout, conv = F32, conv + 1
    if reader_first:
        streak = 0
    for _ in range(n_searches):
        if layout == F32 and (mode == 2 or streak >= RUN):
            layout, conv = SPLIT, conv + 1
        streak += 1
    if reader_last and layout == SPLIT:
        layout, conv = F32, conv + 1
    return layout, conv


def _rank(metric, b):
    rows, q = data(D_E)
    return memo(("rank", metric, b), lambda: oracle.flat_search(metric, rows, q[b], N))


def read_by_id():
    sel = [5, 70, 30000, N - 1]

    def call(ix, metric):
        return ix.search_batch_by_id(np.array(sel, dtype=U64), K_E), 1

    def model(metric, got):
        bd.check(got, bd.expected(metric, data(D_E)[0], sel, K_E), "by id")
    # the gather of the stored rows reads f32 rows (back), then one search at k + 1
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_first=True)


RECOMMEND = [((3, 77, 1000), (20,)), ((65000,), ()), ((5, 6, 7, 8, 9, 40000, 40001), (100, 200, 300))]


def read_recommend():
    def call(ix, metric):
        pos, neg = rd.split(RECOMMEND)
        return ix.recommend_batch(pos, neg, K_E), 1

    def model(metric, got):
        rd.check(got, rd.expected(metric, data(D_E)[0], RECOMMEND, K_E), "recommend")
    # the fold reads the examples as f32 rows (back), then one search at k + 10
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_first=True)


def read_mmr(m):
    def call(ix, metric):
        return ix.search_batch_mmr(data(D_E)[1][:NQ_E], K_E, m, 0.5), 1

    def model(metric, got):
        rows, q = data(D_E)
        md.check(got, md.expected(metric, rows, q[:NQ_E], K_E, m, 0.5), "mmr")
    # one search at depth 40 over the rows as they lie, then the select kernel reads the candidates' f32 rows (back)
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_last=True)


def _code_table(vdb, codes):
    t = vdb.MetaTable(0)
    t.set_codes(0, 0, np.ascontiguousarray(codes, dtype=np.int32))
    t.set_present(0, len(codes), True)
    return t


PG_CODES = (np.arange(N) % 4096).astype(np.int32)                   # 16 or 17 rows a code, spread over the whole store


def read_per_group(vdb, cap):
    from test_gpu_per_group import check as pg_check
    k, g = 5, 3

    def call(ix, metric):
        t = memo("pg table", lambda: _code_table(vdb, PG_CODES))
        ix.debug_set_per_group_scan_cap(cap)
        try:
            got = ix.search_batch_per_group(data(D_E)[1][:NQ_E], k, g, t, 0)
            st = ix.per_group_stats()
        finally:
            ix.debug_set_per_group_scan_cap(0)
        # the route: the member scan (default cap) or one masked search per wanted code (a cap below the 16 members)
        assert (st[2] > 0 and st[3] == 0) if cap == 0 else (st[2] == 0 and st[3] > 0), st
        return got, 1 + (0 if cap == 0 else st[4])

    def model(metric, got):
        pg_check(got, [_rank(metric, b) for b in range(NQ_E)], PG_CODES, k, g, "per group")
    if cap == 0:
        # the search by group (stage A completes: gaussian rows, 4096 codes), then the fill reads f32 rows (back)
        return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_last=True)
    # every code is a giant: the search by group, then one masked search per wanted code; nobody reads f32 rows
    return call, model, lambda mode, start, n: _after_searches(mode, start, n)


def read_grouped():
    ons = np.stack([vf.id_mask(N, 0.01, s, hide=False)[0] for s in (11, 12)])
    words = np.stack([mask_words(on) for on in ons])
    go = np.array([0, 1, vf.GROUP_NONE, 1, 0, vf.GROUP_NONE], dtype=np.uint32)

    def qs():
        return np.ascontiguousarray(data(D_E)[1][:len(go)])

    def call(ix, metric):
        got = ix.search_batch_grouped(qs(), K_E, go, id_masks=words, mask_bits=N)
        st = ix.grouped_stats()
        assert st[0] == len(go) and st[2] == 4 and st[3] == 0 and st[4] == 2, st      # four on the grouped scan, two on the ordinary search
        return got, 1

    def model(metric, got):
        rows, q = data(D_E)[0], qs()
        for b in range(len(go)):
            live = None if go[b] == vf.GROUP_NONE else ons[go[b]].astype(np.uint8)
            check_oracle(metric, rows, q[b:b + 1], K_E, tuple(x[b:b + 1] for x in got), [0], live=live)
    # the grouped scan reads f32 rows (back), then the unfiltered queries take one ordinary search
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_first=True)


def read_range(dense):
    mr = 64

    def radius(metric):
        return rgd.radius_at(_rank(metric, 0), rgd.DENSE_RANK if dense else 6)

    def call(ix, metric):
        got = ix.range_search_batch(data(D_E)[1][:NQ_E], float(radius(metric)), mr)
        st = ix.range_stats()
        assert st[0] + st[1] + st[2] == NQ_E and (st[2] >= 1 if dense else st[0] == NQ_E), st
        return got, 0

    def model(metric, got):
        gi, gd, gc, gt = got
        for b in range(NQ_E):
            oi, od, c, total = rgd.cut(_rank(metric, b), radius(metric), mr)
            assert gc[b] == c and gt[b] == total and np.array_equal(gi[b, :c], oi), (b, gc[b], c, gt[b], total)
            assert np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), b
    # both routes read f32 rows from their first kernel on (vdb_search.cpp range_search: rows_f32 before anything is launched)
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_first=True)


def read_distances():
    lists = [np.array([0, 5, 64, 4095, 30000, N - 1], dtype=U64), np.array([N - 2], dtype=U64), np.arange(100, 164, dtype=U64)]

    def call(ix, metric):
        return tuple(ix.distances_batch(data(D_E)[1][:NQ_E], lists)), 0

    def model(metric, got):
        rows, q = data(D_E)
        for b in range(NQ_E):
            want = np.array([oracle.distance(metric, q[b], rows[int(r)]) for r in lists[b]], dtype=np.float32)
            assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b
    return call, model, lambda mode, start, n: _after_searches(mode, start, n, reader_first=True)


READS = {
    "by_id": lambda vdb: read_by_id(),
    "recommend": lambda vdb: read_recommend(),
    "mmr_40": lambda vdb: read_mmr(40),
    "per_group_fill": lambda vdb: read_per_group(vdb, 0),
    "per_group_giants": lambda vdb: read_per_group(vdb, 4),
    "grouped": lambda vdb: read_grouped(),
    "range_screened": lambda vdb: read_range(False),
    "range_dense": lambda vdb: read_range(True),
    "distances_batch": lambda vdb: read_distances(),
}


@pytest.mark.parametrize("read", list(READS))
@pytest.mark.parametrize("mode", [2, "adaptive"])
@pytest.mark.parametrize("metric", METRICS)
def test_composed_reads(vdb, metric, mode, read):
    rows, queries = data(D_E)
    a, b = pair(vdb, metric, D_E, mode=mode)
    call, model, predict = READS[read](vdb)

    def twin():
        got, _ = call(a, metric)
        model(metric, got)
        return got
    want = memo(("twin", read, metric), twin)
    assert a.layout() == (F32, 0)
    for start in (SPLIT, F32):
        to_split(b, queries)
        if start == F32:
            to_f32(b)
        c0 = b.layout()[1]
        got, searches = call(b, metric)
        end, conv = predict(mode, start, searches)
        seen = (b.layout()[0], b.layout()[1] - c0)
        print(read, metric, mode, "from", start, "predicted", (end, conv), "seen", seen, b.last_stats())
        assert same(want, got), (read, metric, mode, start)
        assert seen == (end, conv), (read, metric, mode, start, "predicted", (end, conv), "seen", seen)


@pytest.mark.parametrize("metric", METRICS)
def test_shadow_switched_on_over_split_rows(vdb, metric):
    """set_shadow(True) builds the bf16 shadow from f32 rows (back); with a shadow the store is no longer split-able"""
    rows, queries = data(D_E)
    q = queries[:9]
    a = pair(vdb, metric, D_E)[0]
    ra = a.search_batch_arrays(q, K_E)
    for mode in (2, "adaptive"):
        b = new_index(vdb, metric, rows, mode)
        to_split(b, queries)
        c0 = b.layout()[1]
        b.set_shadow(True)
        assert b.layout() == (F32, c0 + 1)
        for _ in range(RUN + 2):
            rb = b.search_batch_arrays(q, K_E)
            st = b.last_stats()
            assert st["bf16_screen"] == 1 and st["shadow_rows"] == 1 and b.layout() == (F32, c0 + 1), (st, b.layout())
            assert same(ra, rb)
        b.set_shadow(False)                                        # and without it the layout is tried again
        to_split(b, queries)
        assert same(ra, b.search_batch_arrays(q, K_E))


# ---- the reads that need depth 1024 on the screening tier: at least 240 (1024 + 192) rows
def _large(vdb):
    n = large_n(vdb, 1024)
    return n, data(D_E, n)


def _large_codes(vdb, metric):
    """value_families.distinct_codes over the oracle's ranking of query 0: the ranks 3 .. 199 and 210 .. 1499 share one code, so
    that query 0 sees 4 groups in its first 64 ranks and 14 in its first 1024: k = 8 ends in stage B, k = 16 in stage C"""
    def make():
        n, (rows, q) = _large(vdb)
        rank = oracle.flat_search(metric, rows, q[0], n)
        p = np.arange(n)
        c = (100 + p % 500).astype(np.int32)
        c[p % 97 == 0] = -1
        c[:1500] = vf.DISTINCT_GIANT
        c[[0, 2]] = [10, 12]
        c[1] = -1
        c[200:210] = 20 + np.arange(10)
        codes = np.full(n, -1, dtype=np.int32)
        codes[rank[0].astype(np.int64)] = c
        return codes, rank
    return memo(("large codes", metric), make)


@pytest.mark.parametrize("mode", [2, "adaptive"])
@pytest.mark.parametrize("metric", METRICS)
def test_distinct_and_deep_mmr_at_depth_1024(vdb, metric, mode):
    """One row per group with stage B (depth 1024: rerank_large_kernel over SPLIT rows) and the exclusion rounds of a giant group
    (masked searches at depth 1024), and MMR over 1024 candidates.  At this shape every depth has the sample size 32 768."""
    n, (rows, queries) = _large(vdb)
    q = np.ascontiguousarray(queries[:2])
    codes, rank0 = _large_codes(vdb, metric)
    a, b = (new_index(vdb, metric, rows, m) for m in (0, mode))
    t = _code_table(vdb, codes)
    try:
        for k, stage in ((8, "B"), (16, "C")):
            assert dd.stage_of(rank0, codes, k, n) == stage
            want = a.search_batch_distinct(q[:1], k, t, 0)
            ei, ed, ec = dd.expected(rank0, codes, k)
            assert want[3][0] == k and np.array_equal(want[0][0], ei) and np.array_equal(want[2][0], ec)
            assert np.array_equal(want[1][0].view(np.uint32), ed.view(np.uint32))
            for start in (SPLIT, F32):
                to_split(b, queries)
                if start == F32:
                    to_f32(b)
                c0 = b.layout()[1]
                got = b.search_batch_distinct(q[:1], k, t, 0)
                st = b.distinct_stats()
                assert st[6] == 1024 and (st[2] == 1 if stage == "B" else (st[3] == 1 and st[4] >= 1)), st
                # stage A, stage B and st[4] exclusion searches, all eligible, and nobody reads f32 rows
                end, conv = _after_searches(mode, start, 2 + st[4])
                seen = (b.layout()[0], b.layout()[1] - c0)
                print("distinct", metric, mode, k, "from", start, "predicted", (end, conv), "seen", seen, st, b.last_stats())
                assert same(want, got), (metric, mode, k, start)
                assert seen == (end, conv), (metric, mode, k, start, "predicted", (end, conv), "seen", seen)
        # MMR over 1024 candidates: the search stays on SPLIT rows (the large-k re-rank), the select kernel converts back
        want = a.search_batch_mmr(q, K_E, 1024, 0.5)
        md.check(want, md.expected(metric, rows, q, K_E, 1024, 0.5), "mmr 1024")
        for start in (SPLIT, F32):
            to_split(b, queries)
            if start == F32:
                to_f32(b)
            c0 = b.layout()[1]
            got = b.search_batch_mmr(q, K_E, 1024, 0.5)
            st = b.last_stats()
            assert st["bf16_screen"] == 1 and st["kprime"] > 512 and b.mmr_stats()[1] == 1024, (st, b.mmr_stats())
            end, conv = _after_searches(mode, start, 1, reader_last=True)
            seen = (b.layout()[0], b.layout()[1] - c0)
            print("mmr 1024", metric, mode, "from", start, "predicted", (end, conv), "seen", seen, st)
            assert same(want, got), (metric, mode, start)
            assert seen == (end, conv), (metric, mode, start, "predicted", (end, conv), "seen", seen)
    finally:
        t.close()


# ================================================================== f. two tickets in flight
@pytest.mark.parametrize("metric", METRICS)
def test_a_hand_over_converts_back_with_another_ticket_in_flight(vdb, metric):
    """FORCE_F32 on a SPLIT index, two submitted searches.  Both screening passes read SPLIT rows; waiting on the first hands its
    queries to the f32 tier, which converts back while the second is in flight (convert_rows waits for the whole device first),
    and the second's own hand-over then finds f32 rows."""
    import torch
    d, k, nq = 64, 10, 8
    rows, queries = data(d)
    a, b = pair(vdb, metric, d)
    batches = [np.ascontiguousarray(queries[:nq]), np.ascontiguousarray(queries[nq:2 * nq])]
    ref = [a.search_batch_arrays(x, k) for x in batches]
    to_split(b, queries)
    c0 = b.layout()[1]
    dev = torch.device("cuda", 0)
    qs = [torch.from_numpy(x.copy()).to(dev) for x in batches]
    outs = [(torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    b.set_tiers(b.TIERS_FORCE_F32)
    try:
        t = [b.search_batch_device_submit(qs[i].data_ptr(), nq, d, k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), outs[i][2].data_ptr())
             for i in range(2)]
        assert b.layout() == (SPLIT, c0)
        b.search_batch_device_wait(t[0])
        assert b.layout() == (F32, c0 + 1)
        b.search_batch_device_wait(t[1])
        assert b.layout() == (F32, c0 + 1)
    finally:
        b.set_tiers(0)
    torch.cuda.synchronize()
    for i in range(2):
        got = (outs[i][0].cpu().numpy().view(np.uint64), outs[i][1].cpu().numpy(), outs[i][2].cpu().numpy().astype(np.uintp))
        assert same(ref[i], got), (metric, i)
    check_oracle(metric, rows, batches[1], k, ref[1], [0, nq - 1])


# ================================================================== g. a non-finite element arriving late
@pytest.mark.parametrize("metric", METRICS)
def test_a_non_finite_row_added_to_a_split_index(vdb, metric):
    d, k = 64, 10
    rows, queries = data(d)
    q = queries[:5]
    a, b = (new_index(vdb, metric, rows, m) for m in (0, 2))
    to_split(b, queries)
    c0 = b.layout()[1]
    bad = rows[17].copy()
    bad[3] = np.inf
    late = 10 ** 6

    def run(ix):
        try:
            return ("ok",) + tuple(ix.search_batch_arrays(q, k))
        except Exception as e:                                      # a NaN distance fails the search, as the reference panics
            return ("error", type(e).__name__, str(e))

    def agree(ra, rb):
        assert ra[0] == rb[0], (ra[0], rb[:3])
        assert same(ra[1:], rb[1:]) if ra[0] == "ok" else ra[1:] == rb[1:]

    for ix in (a, b):
        ix.add(late, vdb.Vector(bad))
    ra, rb = run(a), run(b)
    # the append converts back; the search converts forward, finds the element, converts back: three conversions
    assert b.layout() == (F32, c0 + 3), b.layout()
    agree(ra, rb)
    rb2 = run(b)                                                    # refused until the rows change
    assert b.layout() == (F32, c0 + 3)
    agree(ra, rb2)
    for ix in (a, b):
        ix.remove(late)
        ix.compact()
    ra3, rb3 = run(a), run(b)
    assert b.layout() == (SPLIT, c0 + 4), b.layout()               # the rows changed: tried again, and this time it holds
    assert ra3[0] == "ok"
    agree(ra3, rb3)
    check_oracle(metric, rows, q, k, rb3[1:], [0, 4])


# ================================================================== every mutation, under both rules
class GpuSide:
    """a GpuFlatIndex behind the few calls split_schedule.run_schedule makes"""

    def __init__(self, vdb, ix):
        self.vdb, self.ix = vdb, ix
        self.layout, self.last_stats = ix.layout, ix.last_stats

    @staticmethod
    def outcome(call):
        try:
            return ("ok",) + tuple(call())
        except Exception as e:                                      # a NaN distance fails the search, as the reference panics
            return ("error", type(e).__name__, str(e))

    def add(self, id, v):
        self.ix.add(int(id), self.vdb.Vector(v))

    def add_bulk(self, rows, ids):
        self.ix.add_bulk(rows, ids=ids)

    def remove(self, id):
        self.ix.remove(int(id))

    def compact(self, shrink=False):
        self.ix.compact(shrink=shrink)

    def search(self, q, k):
        return self.outcome(lambda: self.ix.search_batch_arrays(q, k))

    def by_id(self, ids, k):
        return self.outcome(lambda: self.ix.search_batch_by_id(np.asarray(ids, dtype=U64), k))

    def capacity(self):
        return self.ix.store_stats()[2]


@pytest.mark.parametrize("mode", [2, "adaptive"])
@pytest.mark.parametrize("metric,d", [(0, 64), (1, 40), (2, 64)])
def test_every_mutation_under_both_rules(vdb, metric, d, mode):
    """tests/split_schedule.py run_schedule over the engine: add, upsert, remove, compact, shrink-compact and refill to the same
    row count, growth across a re-allocation, a fall below 65 536 rows and back, a late non-finite row that is removed again --
    with a plain search (and a read by id) after each, equal to the mode-0 twin and the oracle over the row log, and layout()
    equal to the Rule after EVERY step.  tests/test_split_schedule_cpu.py proves on the CPU that the schedule catches a reader
    that takes the bytes as they lie, an append into split rows and a forgotten refusal."""
    base, queries = data(d)
    a, b = (GpuSide(vdb, new_index(vdb, metric, base, m)) for m in (0, mode))
    rule = run_schedule(a, b, metric, mode, base, queries)
    assert rule.forward >= 6 and rule.back >= 6 and rule.refusals == 1 and b.layout()[0] == SPLIT


# ================================================================== h. the sharded handle
def test_sharded_handle_splits_every_shard(vdb):
    d, k = 64, 10
    n = 3 * N
    rows, queries = data(d, n)
    q = queries[:9]
    plain = new_index(vdb, 0, rows, 0)
    sh = new_index(vdb, 0, rows, 2, devices=[0, 0, 0])
    assert sh.shards() == 3 and all(sh.shard_len(g) >= 65536 for g in range(3))
    assert sh.layout() == (F32, 0)
    want = plain.search_batch_arrays(q, k)
    got = sh.search_batch_arrays(q, k)
    assert sh.layout() == (SPLIT, 3)                                # every child converted, once
    # (the shards answer layout() on their own threads: the sum must not lose one of them, however the threads interleave.  A
    # probabilistic check, on the host alone: the unlocked sum lost a count in one of the first three runs of this test)
    assert {sh.layout() for _ in range(300)} == {(SPLIT, 3)}
    assert same(want, got)
    check_oracle(0, rows, q, k, got, [0, 8])
    ids = np.array([5, N + 70, 2 * N + 30000, n - 1], dtype=U64)     # stored rows of all three shards become queries
    bw, bg = plain.search_batch_by_id(ids, k), sh.search_batch_by_id(ids, k)
    assert same(bw, bg)
    bd.check(bg, bd.expected(0, rows, [int(x) for x in ids], k), "sharded by id")
    assert same(want, sh.search_batch_arrays(q, k)) and sh.layout()[0] == SPLIT

"""One nearest row per group (vdb_flat_search_batch_distinct, csrc/kernels_distinct.hip).  The contract is one
sentence: the full ranking of the eligible rows -- what vdb_flat_search_batch returns under the mask with k = len -- walked from
the front, a row kept iff its group code is -1 or no earlier row has the same code, cut after k kept rows.  Every case compares
ids, order, distance bits, codes and counts with that walk over the CPU oracle's ranking (tests/distinct_data.py;
tests/test_distinct_cpu.py proves which stage of the driver each case ends in)."""
import ctypes

import numpy as np
import pytest

import distinct_data as dd
import range_data as rd
from conftest import load_package

pytestmark = pytest.mark.gpu

U64, F32, I32 = np.uint64, np.float32, np.int32
POISON_ID, POISON_D, POISON_C = U64(0xA5A5A5A5A5A5A5A5), np.uint32(0x7FC0BEEF), I32(-77)


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


_KEEP = {}


def shared(key, make):
    if key not in _KEEP:
        _KEEP[key] = make()
    return _KEEP[key]


def make_index(vdb, metric, rows, ids=None, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(rows, ids=ids)
    return ix


def make_table(vdb, codes, n_present):
    t = vdb.MetaTable(0)
    t.set_codes(0, 0, codes)
    t.set_present(0, n_present, True)
    return t


def chunk_index(vdb, metric):
    return shared(("chunks", metric), lambda: make_index(vdb, metric, dd.chunks()[0]))


def sep_index(vdb, metric):
    return shared(("sep", metric), lambda: make_index(vdb, metric, rd.separated()[0]))


def chunk_table(vdb):
    return shared("chunk table", lambda: make_table(vdb, dd.chunks()[2], dd.CH_N))


def dom_table(vdb):
    return shared("dom table", lambda: make_table(vdb, dd.dominated_codes(), rd.N))


def check(got, ranks, codes, ks, what):
    """got = (ids, dists, codes, counts) against the walk of every query's ranking"""
    gi, gd, gc, gn = got
    for b, rank in enumerate(ranks):
        kb = int(ks if np.isscalar(ks) else ks[b])
        ei, ed, ec = dd.expected(rank, codes, kb)
        c = int(gn[b])
        assert c == len(ei), (what, b, c, len(ei))
        assert np.array_equal(gi[b, :c], ei), (what, b, gi[b, :c], ei)
        assert np.array_equal(gd[b, :c].view(np.uint32), ed.view(np.uint32)), (what, b)
        assert np.array_equal(gc[b, :c], ec), (what, b, gc[b, :c], ec)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def stages(ranks, codes, k, length):
    s = [dd.stage_of(r, codes, k, length) for r in ranks]
    return [s.count("A"), s.count("B"), s.count("C")]


def chunk_ranks(metric):
    rows, q, _ = dd.chunks()
    return [rd.ranking(("distinct chunks", b), metric, rows, q[b]) for b in range(dd.CH_NQ)]


def sep_ranks(metric, key="sep", live=None):
    rows, q, _ = rd.separated()
    return [rd.ranking((key, b), metric, rows, q[b], live=live) for b in range(rd.NQ)]


# ------------------------------------------------------------------ three metrics, every stage
@pytest.mark.parametrize("metric", dd.METRICS)
def test_chunks_end_in_stage_b(vdb, metric):
    _, q, codes = dd.chunks()
    ranks = chunk_ranks(metric)
    ix = chunk_index(vdb, metric)
    got = ix.search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0)
    check(got, ranks, codes, dd.CH_K, "chunks")
    st = ix.distinct_stats()
    a, b, c = stages(ranks, codes, dd.CH_K, dd.CH_N)
    assert st == [dd.CH_NQ, a, b, 0, 0, 40, 1024, dd.CH_NQ * dd.CH_K] and b > 0 and c == 0, st


@pytest.mark.parametrize("metric", dd.METRICS)
def test_dominated_needs_exclusion_rounds(vdb, metric):
    _, q, _ = rd.separated()
    codes = dd.dominated_codes()
    ranks = sep_ranks(metric)
    ix = sep_index(vdb, metric)
    got = ix.search_batch_distinct(q, dd.DOM_K, dom_table(vdb), 0)
    check(got, ranks, codes, dd.DOM_K, "dominated")
    st = ix.distinct_stats()
    a, b, c = stages(ranks, codes, dd.DOM_K, rd.N)
    assert c == 3 and st[:4] == [rd.NQ, a, b, c] and st[4] >= c and st[5:] == [32, 1024, rd.NQ * dd.DOM_K], st
    for j in (3, 7, 11):                                                       # the queries at the 3000-row cluster
        assert got[2][j, 0] == 3 and 3 not in got[2][j, 1:].tolist()


@pytest.mark.parametrize("metric", dd.METRICS)
def test_two_giant_groups_need_two_rounds(vdb, metric):
    """the cluster owns the first 3000 ranks and the background the next 62000: the first exclusion round adds ONE group"""
    _, q, _ = rd.separated()
    codes = dd.giant_codes()
    ranks = sep_ranks(metric)
    ix = sep_index(vdb, metric)
    t = shared("giant table", lambda: make_table(vdb, codes, rd.N))
    got = ix.search_batch_distinct(q[3:4], dd.DOM_K, t, 0)
    check(got, ranks[3:4], codes, dd.DOM_K, "giants")
    assert got[3][0] == 5 and got[2][0, :2].tolist() == [3, dd.GIANT_BG]
    assert ix.distinct_stats() == [1, 0, 0, 1, 2, 32, 1024, 5]
    # k above the number of groups: the count is the number of groups, every group is there
    got = ix.search_batch_distinct(q[:4], 9, t, 0)
    check(got, ranks[:4], codes, 9, "giants, k = 9")
    assert got[3].tolist() == [5, 5, 5, 5] and all(sorted(got[2][b, :5].tolist()) == [0, 1, 2, 3, dd.GIANT_BG] for b in range(4))


# ------------------------------------------------------------------ per-query ks
def raw_distinct(vdb, ix, q, ks, kstride, table, slot=0, k=0, want_codes=True):
    """the C entry point itself, with poisoned outputs: ks an array (k unused) or None (k for every query)"""
    L = vdb._ffi.lib()
    q = np.ascontiguousarray(q, dtype=F32)
    nq, dim = q.shape
    oi = np.full((nq, kstride), POISON_ID, dtype=U64)
    od = np.full((nq, kstride), POISON_D, dtype=np.uint32).view(F32)
    ocode = np.full((nq, kstride), POISON_C, dtype=I32)
    oc = np.full(nq, 12345, dtype=np.uintp)
    u64p, szp, fp, i32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float, ctypes.c_int32))
    ks_ptr = None
    if ks is not None:
        ks = np.ascontiguousarray(ks, dtype=np.uintp)
        ks_ptr = ks.ctypes.data_as(szp)
    rc = L.vdb_flat_search_batch_distinct(ix._h, q.ctypes.data_as(fp), nq, dim, ks_ptr, k, table._t if table is not None else None, slot,
                                          None, 0, kstride, oi.ctypes.data_as(u64p), od.ctypes.data_as(fp),
                                          ocode.ctypes.data_as(i32p) if want_codes else None, oc.ctypes.data_as(szp))
    return rc, oi, od, ocode, oc


@pytest.mark.parametrize("metric", dd.METRICS)
def test_per_query_ks_are_prefixes_of_single_k_calls(vdb, metric):
    _, q, _ = rd.separated()
    codes = dd.dominated_codes()
    ranks = sep_ranks(metric)
    ix = sep_index(vdb, metric)
    ks = np.array([0, 1, 5, 12, 3, 12, 0, 7, 2, 1, 12, 4])
    rc, oi, od, ocode, oc = raw_distinct(vdb, ix, q, ks, 14, dom_table(vdb))
    assert rc == 0, vdb._ffi.last_error()
    check((oi, od, ocode, oc), ranks, codes, ks, "ks")
    for b in range(rd.NQ):
        c = int(oc[b])
        assert c == int(ks[b])
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(np.uint32) == POISON_D).all() and (ocode[b, c:] == POISON_C).all(), b
    single = ix.search_batch_distinct(q, 12, dom_table(vdb), 0)
    for b in range(rd.NQ):
        c = int(ks[b])
        assert np.array_equal(oi[b, :c], single[0][b, :c]) and np.array_equal(od[b, :c].view(np.uint32), single[1][b, :c].view(np.uint32))
    # out_codes may be null
    rc, oi2, od2, _, oc2 = raw_distinct(vdb, ix, q, ks, 14, dom_table(vdb), want_codes=False)
    assert rc == 0 and same((oi, od, oc), (oi2, od2, oc2))


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("metric", dd.METRICS)
def test_host_mask_and_compiled_mask(vdb, metric):
    _, q, _ = rd.separated()
    codes = dd.dominated_codes()
    ok = np.arange(rd.N) % 3 != 1
    ranks = sep_ranks(metric, "sep mod3", ok.astype(np.uint8))
    mask, bits = dd.id_mask(ok)
    ix = sep_index(vdb, metric)
    t = dom_table(vdb)
    a = ix.search_batch_distinct(q, dd.DOM_K, t, 0, id_mask=mask, mask_bits=bits)
    check(a, ranks, codes, dd.DOM_K, "host mask")
    sa = ix.distinct_stats()
    assert sa[3] == 3 and sa[4] >= 3, sa
    # the same filter compiled on the device: slot 1 holds id % 3
    t.set_codes(1, 0, (np.arange(rd.N) % 3).astype(I32))
    with t.compile([(vdb.MetaTable.NE, 1, 1)], rd.N) as cm:
        assert cm.count() == int(ok.sum())
        b = ix.search_batch_distinct(q, dd.DOM_K, t, 0, compiled_mask=cm)
    assert same(a, b) and ix.distinct_stats() == sa


def test_mask_that_removes_a_representative(vdb):
    metric = dd.EUCLID
    rows, q, codes = dd.chunks()
    ranks = chunk_ranks(metric)
    plain = [dd.expected(r, codes, dd.CH_K) for r in ranks]
    ok = np.ones(dd.CH_N, dtype=bool)
    for ei, _, _ in plain:
        ok[ei[::2].astype(np.int64)] = False                                   # every other representative of every answer goes
    masked = [rd.ranking(("distinct chunks minus reps", b), metric, rows, q[b], live=ok.astype(np.uint8)) for b in range(dd.CH_NQ)]
    mask, bits = dd.id_mask(ok)
    got = chunk_index(vdb, metric).search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0, id_mask=mask, mask_bits=bits)
    check(got, masked, codes, dd.CH_K, "representatives removed")
    moved = 0
    for b, (ei, _, ec) in enumerate(plain):
        for i in range(0, dd.CH_K, 2):                                         # the group is still answered, by its next row
            at = np.nonzero(got[2][b] == ec[i])[0]
            if at.size:
                assert got[0][b, at[0]] != ei[i] and codes[int(got[0][b, at[0]])] == ec[i]
                moved += 1
    assert moved > dd.CH_NQ


def test_mask_leaving_fewer_than_k_groups(vdb):
    metric = dd.COSINE
    rows, q, members = rd.separated()
    codes = dd.dominated_codes()
    ok = np.zeros(rd.N, dtype=bool)
    for m in members:
        ok[m] = True                                                           # the four clusters only ...
    lone = np.nonzero(codes == -1)[0][:2]
    ok[lone] = True                                                            # ... and two rows without a group: six groups
    ranks = sep_ranks(metric, "sep clusters + 2", ok.astype(np.uint8))
    mask, bits = dd.id_mask(ok)
    ix = sep_index(vdb, metric)
    got = ix.search_batch_distinct(q, 10, dom_table(vdb), 0, id_mask=mask, mask_bits=bits)
    check(got, ranks, codes, 10, "six groups")
    assert got[3].tolist() == [6] * rd.NQ
    for b in range(rd.NQ):
        assert sorted(got[2][b, :6].tolist()) == [-1, -1, 0, 1, 2, 3] and set(lone.tolist()) <= set(got[0][b, :6].tolist())
    st = ix.distinct_stats()
    assert st[0] == rd.NQ and st[1] + st[2] + st[3] == rd.NQ and st[3] >= 3 and st[7] == 6 * rd.NQ, st


def test_rows_without_a_group_are_singletons_until_an_exists_filter(vdb):
    metric = dd.EUCLID
    _, q, _ = rd.separated()
    codes = dd.dominated_codes()
    ranks = sep_ranks(metric)
    ix = sep_index(vdb, metric)
    t = dom_table(vdb)
    k = 120                                                                    # 54 groups at most: the rest of an answer is -1 rows
    got = ix.search_batch_distinct(q, k, t, 0)
    check(got, ranks, codes, k, "singletons")
    for b in range(rd.NQ):
        c = got[2][b]
        assert got[3][b] == k and (c == -1).sum() >= k - 54 and len(set(c[c != -1].tolist())) == (c != -1).sum()
    has = codes != -1
    with_field = sep_ranks(metric, "sep has code", has.astype(np.uint8))
    with t.compile([(vdb.MetaTable.EXISTS, 0, 0)], rd.N) as cm:
        got = ix.search_batch_distinct(q, k, t, 0, compiled_mask=cm)
    check(got, with_field, codes, k, "exists")
    assert got[3].tolist() == [54] * rd.NQ and all((got[2][b, :54] != -1).all() for b in range(rd.NQ))


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", dd.METRICS)
@pytest.mark.parametrize("shared_code", [True, False])
def test_tied_rows(vdb, metric, shared_code):
    rows, q = rd.tied()
    codes = dd.tied_codes(shared_code)
    ranks = [rd.ranking(("tied", 0), metric, rows, q[0])]
    ix = shared(("tied", metric), lambda: make_index(vdb, metric, rows))
    t = make_table(vdb, codes, rd.N)
    got = ix.search_batch_distinct(q[:1], 5, t, 0)
    check(got, ranks, codes, 5, "tied")
    first = got[0][0].tolist()
    if shared_code:
        assert first[0] == min(rd.TIE_ROWS) and not set(first[1:]) & set(rd.TIE_ROWS)
    else:
        assert first == sorted(rd.TIE_ROWS) and len(set(got[1][0].view(np.uint32).tolist())) == 1
    t.close()


# ------------------------------------------------------------------ the other tiers
@pytest.mark.parametrize("metric", dd.METRICS)
def test_small_index_direct_path_and_without_it(vdb, metric):
    rows, q, codes = dd.small()
    ranks = [rd.ranking(("distinct small", b), metric, rows, q[b]) for b in range(dd.SM_NQ)]
    ix = make_index(vdb, metric, rows)
    t = make_table(vdb, codes, dd.SM_N)
    for k in (7, 60, 300):                                                     # 300: dA = dB = 1024, more than the 37 codes + the -1 rows nearby
        a = ix.search_batch_distinct(q, k, t, 0)
        check(a, ranks, codes, k, ("small", k))
        assert (a[2][a[0] >= U64(dd.SM_COL)] == -1).all()                       # ids beyond the column have no group
        ix.set_tiers(vdb.GpuFlatIndex.TIERS_NO_DIRECT)
        b = ix.search_batch_distinct(q, k, t, 0)
        ix.set_tiers(0)
        assert same(a, b), k
    # fewer rows than any depth: one search sees everything
    tiny = make_index(vdb, metric, rows[:20])
    got = tiny.search_batch_distinct(q, 25, t, 0)
    check(got, [rd.ranking(("distinct small 20", b), metric, rows[:20], q[b]) for b in range(dd.SM_NQ)], codes, 25, "tiny")
    assert tiny.distinct_stats()[:7] == [dd.SM_NQ, dd.SM_NQ, 0, 0, 0, 20, 20]
    t.close()


def test_chunks_under_the_exact_scan(vdb):
    _, q, codes = dd.chunks()
    ix = chunk_index(vdb, dd.EUCLID)
    a = ix.search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0)
    ix.set_tiers(vdb.GpuFlatIndex.TIERS_FORCE_EXACT)
    try:
        b = ix.search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0)
        assert ix.last_stats()["exact_queries"] > 0
    finally:
        ix.set_tiers(0)
    check(b, chunk_ranks(dd.EUCLID), codes, dd.CH_K, "exact scan")
    assert same(a, b)


@pytest.mark.parametrize("metric", dd.METRICS)
def test_sharded_handle(vdb, metric):
    rows, q, _ = rd.separated()
    codes = dd.dominated_codes()
    sh = make_index(vdb, metric, rows, devices=[0, 0, 0])
    assert sh.shards() == 3
    got = sh.search_batch_distinct(q, dd.DOM_K, dom_table(vdb), 0)
    check(got, sep_ranks(metric), codes, dd.DOM_K, "sharded")
    ix = sep_index(vdb, metric)
    assert same(got, ix.search_batch_distinct(q, dd.DOM_K, dom_table(vdb), 0))
    assert sh.distinct_stats() == ix.distinct_stats()
    ok = np.arange(rd.N) % 3 != 1
    mask, bits = dd.id_mask(ok)
    ks = np.array([5, 1, 0, 9] * 3)
    got = sh.search_batch_distinct(q, ks, dom_table(vdb), 0, id_mask=mask, mask_bits=bits)
    check(got, sep_ranks(metric, "sep mod3", ok.astype(np.uint8)), codes, ks, "sharded, masked, ks")


# ------------------------------------------------------------------ staged writes
def test_column_written_after_a_search(vdb):
    metric = dd.EUCLID
    rows, q, codes = dd.small()
    ranks = [rd.ranking(("distinct small", b), metric, rows, q[b]) for b in range(dd.SM_NQ)]
    ix = make_index(vdb, metric, rows)
    t = make_table(vdb, codes, dd.SM_N)
    check(ix.search_batch_distinct(q, 20, t, 0), ranks, codes, 20, "before")
    # a staged column write (longer than before: the device copy moves) and a staged add reach the device before the next search
    codes2 = ((np.arange(dd.SM_N + 1) * 7) % 23).astype(I32)
    t.set_codes(0, 0, codes2)
    extra = (q[0] + F32(1e-3)).astype(F32)
    ix.add(dd.SM_N, vdb.Vector(extra))
    rows2 = np.concatenate([rows, extra[None, :]])
    ranks2 = [rd.ranking(("distinct small + 1", b), metric, rows2, q[b]) for b in range(dd.SM_NQ)]
    got = ix.search_batch_distinct(q, 20, t, 0)
    check(got, ranks2, codes2, 20, "after")
    assert got[0][0, 0] == dd.SM_N and got[2][0, 0] == codes2[dd.SM_N]
    # a single-row write
    t.set_codes(0, dd.SM_N, np.array([-1], dtype=I32))
    codes2[dd.SM_N] = -1
    check(ix.search_batch_distinct(q, 20, t, 0), ranks2, codes2, 20, "one row")
    t.close()


# ------------------------------------------------------------------ errors
def test_errors_come_before_any_search(vdb):
    E = vdb._ffi.ERR_INVALID_ARGUMENT
    rows, q, codes = dd.small()
    ix = make_index(vdb, dd.EUCLID, rows)
    t = make_table(vdb, codes, dd.SM_N)
    ix.search_batch_arrays(q, 3)
    before = ix.last_stats()

    def refused(rc_and_outputs, what):
        rc, oi, _, _, oc = rc_and_outputs
        assert rc == E, (what, rc, vdb._ffi.last_error())
        assert (oc == 12345).all() and (oi == POISON_ID).all() and ix.last_stats() == before, what

    refused(raw_distinct(vdb, ix, q, None, 4, None, k=4), "null table")
    refused(raw_distinct(vdb, ix, q, None, 4, t, slot=3, k=4), "unknown slot")
    refused(raw_distinct(vdb, ix, q, None, 1025, t, k=1025), "k above 1024")
    refused(raw_distinct(vdb, ix, q, np.array([1, 2, 1025, 1, 1]), 1025, t), "max(ks) above 1024")
    refused(raw_distinct(vdb, ix, q, None, 3, t, k=4), "kstride below k")
    for call in (lambda: ix.search_batch_distinct(q, 4, None, 0), lambda: ix.search_batch_distinct(q, 4, t, 9),
                 lambda: ix.search_batch_distinct(q, 1025, t, 0)):
        with pytest.raises(vdb.IndexError_):
            call()
    rc, oi, od, ocode, oc = raw_distinct(vdb, ix, q, None, 1024, t, k=1024)    # 1024 itself is served
    assert rc == 0
    check((oi, od, ocode, oc), [rd.ranking(("distinct small", b), dd.EUCLID, rows, q[b]) for b in range(dd.SM_NQ)], codes, 1024, "k = 1024")
    before = ix.last_stats()
    # k = 0 and an empty index: counts 0 before any check
    rc, _, _, _, oc = raw_distinct(vdb, ix, q, None, 1, None, k=0)
    assert rc == 0 and (oc == 0).all() and ix.last_stats() == before
    empty = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    rc, _, _, _, oc = raw_distinct(vdb, empty, q, None, 4, None, k=4)
    assert rc == 0 and (oc == 0).all() and empty.distinct_stats() == [dd.SM_NQ, 0, 0, 0, 0, 0, 0, 0]
    # the error of the equivalent search
    with pytest.raises(vdb.DimensionMismatch) as e1:
        ix.search_batch_arrays(q[:, :5], 3)
    with pytest.raises(vdb.DimensionMismatch) as e2:
        ix.search_batch_distinct(q[:, :5], 3, t, 0)
    assert (e1.value.expected, e1.value.actual) == (e2.value.expected, e2.value.actual)
    # a sharded handle refuses alike
    sh = make_index(vdb, dd.EUCLID, rows[:600], devices=[0, 0])
    for rc_out in (raw_distinct(vdb, sh, q, None, 4, None, k=4), raw_distinct(vdb, sh, q, None, 4, t, slot=3, k=4),
                   raw_distinct(vdb, sh, q, None, 1025, t, k=1025)):
        assert rc_out[0] == E and (rc_out[4] == 12345).all()
    t.close()


def test_cosine_errors_are_those_of_the_search(vdb):
    rows, q, codes = dd.small()
    t = make_table(vdb, codes, dd.SM_N)
    ix = make_index(vdb, dd.COSINE, rows)
    ix.add(dd.SM_N, vdb.Vector(np.zeros(dd.SM_D, dtype=F32)))                  # a zero-norm row fails every search
    with pytest.raises(vdb.InvalidVector):
        ix.search_batch_arrays(q, 5)
    with pytest.raises(vdb.InvalidVector):
        ix.search_batch_distinct(q, 5, t, 0)
    ix.remove(dd.SM_N)
    zq = q.copy()
    zq[2] = 0                                                                  # ... and so does a zero-norm query
    with pytest.raises(vdb.InvalidVector):
        ix.search_batch_distinct(zq, 5, t, 0)
    bad = rows[3].copy()
    bad[2] = np.nan
    ix.add(dd.SM_N + 1, vdb.Vector(bad))
    with pytest.raises(vdb.NanDistance):
        ix.search_batch_distinct(q, 5, t, 0)
    ix.remove(dd.SM_N + 1)
    ranks = [rd.ranking(("distinct small", b), dd.COSINE, rows, q[b]) for b in range(dd.SM_NQ)]
    check(ix.search_batch_distinct(q, 5, t, 0), ranks, codes, 5, "after the bad rows left")
    t.close()


def test_refused_while_a_ticket_is_outstanding(vdb):
    import torch
    rows, q, codes = dd.chunks()
    ix = make_index(vdb, dd.EUCLID, rows)                                      # (its own handle: a ticket blocks every other caller)
    dev = torch.device("cuda", 0)
    B, k = 16, 10
    dq = torch.from_numpy(rows[:B].copy()).to(dev)
    out = (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev))
    ticket = ix.search_batch_device_submit(dq.data_ptr(), B, dd.CH_D, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    try:
        with pytest.raises(vdb.VectorDbError):
            ix.search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0)
    finally:
        ix.search_batch_device_wait(ticket)
    torch.cuda.synchronize()
    check(ix.search_batch_distinct(q, dd.CH_K, chunk_table(vdb), 0), chunk_ranks(dd.EUCLID), codes, dd.CH_K, "after the ticket")


def test_an_id_at_or_above_2_to_32_is_refused_for_good(vdb):
    E = vdb._ffi.ERR_INVALID_ARGUMENT
    rows, q, codes = dd.small()
    t = make_table(vdb, codes, dd.SM_N)
    for top, fine in ((2 ** 32, False), (2 ** 32 - 1, True)):
        for kw in ({}, {"devices": [0, 0]}):
            ids = np.arange(40, dtype=U64)
            ids[17] = U64(top)
            ix = make_index(vdb, dd.EUCLID, rows[:40], ids=ids, **kw)
            rc, _, _, _, oc = raw_distinct(vdb, ix, q, None, 4, t, k=4)
            if fine:                                                           # 2^32 - 1 is an ordinary id: no code, its own group
                assert rc == 0 and (oc == 4).all()
                ranks = [rd.ranking(("distinct small 40 top", b), dd.EUCLID, rows[:40], q[b], ids=ids) for b in range(dd.SM_NQ)]
                check(ix.search_batch_distinct(q, 40, t, 0), ranks, codes, 40, ("id 2^32 - 1", kw))
                continue
            assert rc == E and (oc == 12345).all(), (top, kw, rc)
            ix.remove(top)                                                     # the running maximum is never lowered
            assert ix.len() == 39
            assert raw_distinct(vdb, ix, q, None, 4, t, k=4)[0] == E
    t.close()


def test_table_on_another_device(vdb):
    try:
        t = vdb.MetaTable(1)
    except vdb.IndexError_ as e:
        assert "out of range" in str(e)
        pytest.skip("needs a second GPU to hold the table")
    rows, q, codes = dd.small()
    ix = make_index(vdb, dd.EUCLID, rows)
    t.set_codes(0, 0, codes)
    assert raw_distinct(vdb, ix, q, None, 4, t, k=4)[0] == vdb._ffi.ERR_INVALID_ARGUMENT
    t.close()


# ------------------------------------------------------------------ the store
def test_store_search_distinct(vdb):
    F = vdb.MetadataFilter
    n, d, k = 600, 16, 8
    rng = np.random.default_rng(20263)
    rows = rng.standard_normal((n, d)).astype(F32)
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    doc = [None if i % 13 == 0 else f"doc-{(i * 7) % 40}" for i in range(n)]  # 40 documents; every 13th row has none
    lang = [("en", "de", "fr")[i % 3] for i in range(n)]
    with pytest.raises(ValueError):
        st.search_distinct(vdb.Vector(rows[0]), k, "doc")                       # the device table is required
    st.set_device_filter(True)
    half = n // 2
    for i in range(half):
        meta = {"lang": lang[i]}
        if doc[i] is not None:
            meta["doc"] = doc[i]
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata(meta))
    st.index().add_bulk(rows[half:], first_id=half)
    st.attach_bulk_metadata(n - half, {"doc": doc[half:], "lang": lang[half:]}, ids=[f"bulk-{i}" for i in range(half, n)])
    name = lambda i: f"item-{i}" if i < half else f"bulk-{i}"
    queries = [vdb.Vector((rows[i] + F32(0.01)).astype(F32)) for i in (3, 13, 299, 300, 599, 26, 77, 400, 401)]

    def restated(qv, k, ok):
        """the walk in numpy over the store's own metadata"""
        d2 = np.sqrt(((rows.astype(np.float64) - qv.data.astype(np.float64)) ** 2).sum(axis=1))
        seen, out = set(), []
        for i in np.lexsort((np.arange(n), d2)):
            if not ok[i] or (doc[i] is not None and doc[i] in seen):
                continue
            seen.add(doc[i])
            out.append(name(int(i)))
            if len(out) == k:
                break
        return out

    everyone = np.ones(n, dtype=bool)
    german_with_doc = np.array([lang[i] == "de" and doc[i] is not None for i in range(n)])
    for flt, ok in ((None, everyone), (F.And([F.Eq("lang", "de"), F.Exists("doc")]), german_with_doc)):
        got = st.search_distinct_batch(queries, k, "doc", flt)
        for b, qv in enumerate(queries):
            assert [r.id for r in got[b]] == restated(qv, k, ok), (b, flt is not None)
        one = st.search_distinct(queries[2], k, "doc", flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[2]]
    assert len(st.search_distinct(queries[0], 100, "doc", F.Exists("doc"))) == 40
    # a field nobody has: every row is its own group -- the plain search
    plain = st.search(queries[0], k)
    assert [(r.id, r.distance) for r in st.search_distinct(queries[0], k, "nobody-has-this")] == [(r.id, r.distance) for r in plain]

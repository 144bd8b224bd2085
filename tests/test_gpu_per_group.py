"""The k nearest groups with up to g rows of each (vdb_flat_search_batch_per_group, csrc/kernels_per_group.hip).
The contract: the GROUPS are vdb_flat_search_batch_distinct's answer; the MEMBERS of a group with code c >= 0 are the first g rows
of the full ranking of the eligible rows whose code is c; a row with code -1 is its own group of one.  Every case compares ids,
order, distance bits, codes, sizes and counts with that sentence executed in numpy over the CPU oracle's ranking
(tests/per_group_data.py; tests/test_per_group_cpu.py proves what the families are assumed to do)."""
import ctypes

import numpy as np
import pytest

import distinct_data as dd
import per_group_data as pg
import range_data as rd
from conftest import load_package

pytestmark = pytest.mark.gpu

U64, F32, I32, U32 = np.uint64, np.float32, np.int32, np.uint32
POISON_ID, POISON_D, POISON_C, POISON_S = U64(0xA5A5A5A5A5A5A5A5), U32(0x7FC0BEEF), I32(-77), U32(0xDEAD)


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


def scat_index(vdb, metric):
    return shared(("scattered", metric), lambda: make_index(vdb, metric, pg.scattered()[0]))


def scat_table(vdb):
    return shared("scattered table", lambda: make_table(vdb, pg.scattered()[2], pg.SC_N))


def scat_ranks(metric, key="per group scattered", live=None, rows=None):
    r, q, _ = pg.scattered()
    return [rd.ranking((key, b), metric, r if rows is None else rows, q[b], live=live) for b in range(pg.SC_NQ)]


def sep_index(vdb, metric):
    return shared(("sep", metric), lambda: make_index(vdb, metric, rd.separated()[0]))


def sep_ranks(metric):
    rows, q, _ = rd.separated()
    return [rd.ranking(("sep", b), metric, rows, q[b]) for b in range(rd.NQ)]


def check(got, ranks, codes, ks, g, what):
    """got = (ids [nq, k, g], dists, codes [nq, k], sizes [nq, k], counts) against the model of every query"""
    gi, gd, gc, gs, gn = got
    for b, rank in enumerate(ranks):
        kb = int(ks if np.isscalar(ks) else ks[b])
        want = pg.expected(rank, codes, kb, g)
        assert int(gn[b]) == len(want), (what, b, int(gn[b]), len(want))
        for j, (code, ids, dists) in enumerate(want):
            m = int(gs[b, j])
            assert gc[b, j] == code and m == len(ids), (what, b, j, gc[b, j], code, m, len(ids))
            assert np.array_equal(gi[b, j, :m], ids), (what, b, j, gi[b, j, :m], ids)
            assert np.array_equal(gd[b, j, :m].view(U32), dists.view(U32)), (what, b, j)


def same(a, b):
    """two answers agree on everything the contract calls meaningful"""
    if not (np.array_equal(a[4], b[4]) and all(np.array_equal(a[3][q, :int(c)], b[3][q, :int(c)]) for q, c in enumerate(a[4]))):
        return False
    for q, c in enumerate(a[4]):
        for j in range(int(c)):
            m = int(a[3][q, j])
            if a[2][q, j] != b[2][q, j] or not np.array_equal(a[0][q, j, :m], b[0][q, j, :m]) or \
                    not np.array_equal(a[1][q, j, :m].view(U32), b[1][q, j, :m].view(U32)):
                return False
    return True


def raw(vdb, ix, q, ks, kstride, g, table, slot=0, k=0, want_sizes=True, want_ids=True, gdim=None):
    """the C entry point itself, with poisoned outputs: ks an array (k unused) or None (k for every query)"""
    L = vdb._ffi.lib()
    q = np.ascontiguousarray(q, dtype=F32)
    nq, dim = q.shape
    gdim = max(g, 1) if gdim is None else gdim
    oi = np.full((nq, kstride, gdim), POISON_ID, dtype=U64)
    od = np.full((nq, kstride, gdim), POISON_D, dtype=U32).view(F32)
    ocode = np.full((nq, kstride), POISON_C, dtype=I32)
    osz = np.full((nq, kstride), POISON_S, dtype=U32)
    oc = np.full(nq, 12345, dtype=np.uintp)
    u64p, szp, fp, i32p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float, ctypes.c_int32, ctypes.c_uint32))
    ks_ptr = None
    if ks is not None:
        ks = np.ascontiguousarray(ks, dtype=np.uintp)
        ks_ptr = ks.ctypes.data_as(szp)
    rc = L.vdb_flat_search_batch_per_group(ix._h, q.ctypes.data_as(fp), nq, dim, ks_ptr, k, g, table._t if table is not None else None, slot,
                                           None, 0, kstride, oi.ctypes.data_as(u64p) if want_ids else None, od.ctypes.data_as(fp),
                                           ocode.ctypes.data_as(i32p), osz.ctypes.data_as(u32p) if want_sizes else None, oc.ctypes.data_as(szp))
    return rc, (oi, od, ocode, osz, oc)


def untouched(out):
    oi, od, ocode, osz, oc = out
    return bool((oi == POISON_ID).all() and (od.view(U32) == POISON_D).all() and (ocode == POISON_C).all() and (osz == POISON_S).all()
                and (oc == 12345).all())


# ------------------------------------------------------------------ three metrics, every group size
@pytest.mark.parametrize("metric", pg.METRICS)
def test_scattered_every_group_size(vdb, metric):
    _, q, codes = pg.scattered()
    ranks = scat_ranks(metric)
    ix, t = scat_index(vdb, metric), scat_table(vdb)
    for g in (3, 1, 2, 32):                                                   # 32: a document has 8 rows, every group is smaller than g
        got = ix.search_batch_per_group(q, pg.SC_K, g, t, 0)
        check(got, ranks, codes, pg.SC_K, g, ("scattered", g))
        st = ix.per_group_stats()
        assert st == [pg.SC_NQ] + pg.routes(ranks, codes, pg.SC_K, g) + [0], (g, st)
        if g == 32:
            assert (got[3] == pg.SC_PER).all()
        if g == 1:                                                             # distinct's own answer, bit for bit, every size 1
            di, dv, dc, dn = ix.search_batch_distinct(q, pg.SC_K, t, 0)
            assert np.array_equal(dn, got[4]) and np.array_equal(di, got[0][:, :, 0]) and np.array_equal(dc, got[2])
            assert np.array_equal(dv.view(U32), got[1][:, :, 0].view(U32)) and (got[3] == 1).all()


# ------------------------------------------------------------------ long lists, both routes
@pytest.mark.parametrize("metric", pg.METRICS)
@pytest.mark.parametrize("family", ["dominated", "giants"])
def test_long_lists_on_both_routes(vdb, metric, family):
    _, q, _ = rd.separated()
    codes = dd.dominated_codes() if family == "dominated" else dd.giant_codes()
    ranks = sep_ranks(metric)
    ix = sep_index(vdb, metric)
    t = shared((family, "table"), lambda: make_table(vdb, codes, rd.N))
    g = pg.SC_G
    a = ix.search_batch_per_group(q, dd.DOM_K, g, t, 0)
    check(a, ranks, codes, dd.DOM_K, g, (family, "default cap"))
    st = ix.per_group_stats()
    assert st == [rd.NQ] + pg.routes(ranks, codes, dd.DOM_K, g) + [0] and st[3] == 0 and st[2] > 0, st
    assert ix.distinct_stats()[3] > 0                                          # stage C of the search by group ran in front
    ix.debug_set_per_group_scan_cap(pg.LOW_CAP)
    try:
        b = ix.search_batch_per_group(q, dd.DOM_K, g, t, 0)
        st = ix.per_group_stats()
    finally:
        ix.debug_set_per_group_scan_cap(0)
    assert st == [rd.NQ] + pg.routes(ranks, codes, dd.DOM_K, g, pg.LOW_CAP) + [0] and st[2] > 0 and st[3] > 0, st
    check(b, ranks, codes, dd.DOM_K, g, (family, "cap 1024"))
    assert same(a, b)


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", pg.METRICS)
def test_tied_rows(vdb, metric):
    rows, q = rd.tied()
    codes = dd.tied_codes(True)
    ranks = [rd.ranking(("tied", 0), metric, rows, q[0])]
    ix = shared(("tied", metric), lambda: make_index(vdb, metric, rows))
    t = shared("tied table", lambda: make_table(vdb, codes, rd.N))
    got = ix.search_batch_per_group(q[:1], 5, 3, t, 0)
    check(got, ranks, codes, 5, 3, "tied, g = 3")
    assert got[0][0, 0].tolist() == sorted(rd.TIE_ROWS)[:3] and len(set(got[1][0, 0].view(U32).tolist())) == 1
    got = ix.search_batch_per_group(q[:1], 5, 8, t, 0)
    check(got, ranks, codes, 5, 8, "tied, g = 8")
    assert got[3][0, 0] == 5 and got[0][0, 0, :5].tolist() == sorted(rd.TIE_ROWS)


# ------------------------------------------------------------------ small indexes
@pytest.mark.parametrize("metric", pg.METRICS)
def test_small_indexes(vdb, metric):
    rows, q, codes = dd.small()                                                # a column shorter than the id range, -1 codes, the direct path
    ranks = [rd.ranking(("distinct small", b), metric, rows, q[b]) for b in range(dd.SM_NQ)]
    ix = make_index(vdb, metric, rows)
    t = make_table(vdb, codes, dd.SM_N)
    for k, g in ((7, 2), (60, 3), (300, 32)):
        got = ix.search_batch_per_group(q, k, g, t, 0)
        check(got, ranks, codes, k, g, ("small", k, g))
        lone = got[2] == -1
        assert (got[3][lone & (np.arange(got[2].shape[1])[None, :] < got[4][:, None])] == 1).all()
    assert ix.per_group_stats()[1:] == pg.routes(ranks, codes, 300, 32) + [0]
    t.close()
    rows, q, codes = pg.odd()                                                  # 33 elements a row: the row pitch is not the dimension
    ranks = [rd.ranking(("per group odd", b), metric, rows, q[b]) for b in range(pg.ODD_NQ)]
    ix = make_index(vdb, metric, rows)
    t = make_table(vdb, codes, pg.ODD_N)
    for k, g in ((5, 3), (40, 32)):
        check(ix.search_batch_per_group(q, k, g, t, 0), ranks, codes, k, g, ("odd", k, g))
    t.close()


# ------------------------------------------------------------------ per-query ks
def test_per_query_ks_are_prefixes(vdb):
    metric = dd.EUCLID
    _, q, codes = pg.scattered()
    ranks = scat_ranks(metric)
    ix, t = scat_index(vdb, metric), scat_table(vdb)
    ks = np.array([0, 1, 5, 12, 3, 12, 0, 7, 2, 1, 12, 4])
    g = 3
    rc, out = raw(vdb, ix, q, ks, 14, g, t)
    assert rc == 0, vdb._ffi.last_error()
    check(out, ranks, codes, ks, g, "ks")
    assert ix.per_group_stats() == [pg.SC_NQ] + pg.routes(ranks, codes, ks, g) + [0]
    oi, od, ocode, osz, oc = out
    single = ix.search_batch_per_group(q, 12, g, t, 0)
    for b in range(pg.SC_NQ):
        c = int(oc[b])
        assert c == int(ks[b])
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(U32) == POISON_D).all() and (osz[b, c:] == POISON_S).all(), b
        assert np.array_equal(oi[b, :c], single[0][b, :c]) and np.array_equal(od[b, :c].view(U32), single[1][b, :c].view(U32))
        assert np.array_equal(osz[b, :c], single[3][b, :c]) and np.array_equal(ocode[b, :c], single[2][b, :c])


# ------------------------------------------------------------------ masks, host and compiled
@pytest.mark.parametrize("metric", pg.METRICS)
def test_masks_that_remove_members_and_empty_a_group(vdb, metric):
    rows, q, codes = pg.scattered()
    ranks = scat_ranks(metric)
    ix, t = scat_index(vdb, metric), scat_table(vdb)
    k, g = pg.SC_K, pg.SC_G
    ok = np.ones(pg.SC_N, dtype=bool)
    emptied = []
    for b, rank in enumerate(ranks):
        plain = pg.expected(rank, codes, k, g)
        ok[int(plain[0][1][0])] = False                                        # the nearest group loses its representative ...
        ok[int(plain[0][1][2])] = False                                        # ... and another member
        ok[codes == plain[1][0]] = False                                       # the second group loses every row
        emptied.append(plain[1][0])
    masked = scat_ranks(metric, "per group scattered masked", ok.astype(np.uint8))
    mask, bits = dd.id_mask(ok)
    a = ix.search_batch_per_group(q, k, g, t, 0, id_mask=mask, mask_bits=bits)
    check(a, masked, codes, k, g, "host mask")
    for b in range(pg.SC_NQ):
        assert emptied[b] not in a[2][b].tolist() and ok[a[0][b][np.arange(g)[None, :] < a[3][b][:, None]].astype(np.int64)].all()
    sa = ix.per_group_stats()
    assert sa == [pg.SC_NQ] + pg.routes(masked, codes, k, g) + [0]
    # the same filter compiled on the device: slot 1 holds "masked out"
    t.set_codes(1, 0, (~ok).astype(I32))
    with t.compile([(vdb.MetaTable.NE, 1, 1)], pg.SC_N) as cm:
        assert cm.count() == int(ok.sum())
        b = ix.search_batch_per_group(q, k, g, t, 0, compiled_mask=cm)
    assert same(a, b) and ix.per_group_stats() == sa
    # under the low cap the giants' route searches under "mask AND code == c"
    ix.debug_set_per_group_scan_cap(4)
    try:
        c = ix.search_batch_per_group(q, k, g, t, 0, id_mask=mask, mask_bits=bits)
        st = ix.per_group_stats()
    finally:
        ix.debug_set_per_group_scan_cap(0)
    assert same(a, c) and st[3] > 0 and st[2] == 0, st


# ------------------------------------------------------------------ removed rows, re-added ids, compaction
def test_removed_and_readded_rows_and_compaction(vdb):
    metric = dd.COSINE
    rows, q, codes = pg.scattered()
    ranks = scat_ranks(metric)
    k, g = pg.SC_K, pg.SC_G
    ix = make_index(vdb, metric, rows)                                         # (its own handle: it is mutated)
    t = scat_table(vdb)
    rows2 = rows.copy()
    live = np.ones(pg.SC_N, dtype=np.uint8)
    for b in range(0, pg.SC_NQ, 2):
        plain = pg.expected(ranks[b], codes, k, g)
        gone = int(plain[0][1][1])                                             # the second member of the nearest group leaves
        ix.remove(gone)
        live[gone] = 0
        back = int(plain[1][1][2])                                             # the third member of the second group comes back next to the query
        ix.remove(back)
        rows2[back] = q[b] + F32(0.01)
        ix.add(back, vdb.Vector(rows2[back]))
    after = scat_ranks(metric, "per group scattered mutated", live, rows2)
    got = ix.search_batch_per_group(q, k, g, t, 0)
    check(got, after, codes, k, g, "after removes and re-adds")
    for b in range(0, pg.SC_NQ, 2):
        plain = pg.expected(ranks[b], codes, k, g)
        members = got[0][b][np.arange(g)[None, :] < got[3][b][:, None]].tolist()
        assert int(plain[0][1][1]) not in members and got[0][b, 0, 0] == plain[1][1][2]   # the re-added row is now the nearest of all
    assert ix.compact() > 0
    again = ix.search_batch_per_group(q, k, g, t, 0)
    check(again, after, codes, k, g, "after compact")
    assert same(got, again)


# ------------------------------------------------------------------ the SPLIT layout
def test_split_layout_is_converted_back(vdb):
    metric = dd.EUCLID
    _, q, codes = pg.scattered()
    ix, t = scat_index(vdb, metric), scat_table(vdb)
    k, g = pg.SC_K, pg.SC_G
    before = ix.search_batch_per_group(q, k, g, t, 0)
    ix.set_split(2)
    try:
        ix.search_batch_arrays(q, 10)                                          # one screened search converts the rows
        assert ix.layout()[0] == 1
        got = ix.search_batch_per_group(q, k, g, t, 0)
        assert ix.layout()[0] == 0                                             # the fill read plain f32 rows
    finally:
        ix.set_split(1)
    check(got, scat_ranks(metric), codes, k, g, "split")
    assert same(before, got)


# ------------------------------------------------------------------ errors
def test_errors_leave_the_outputs_untouched(vdb):
    E = vdb._ffi.ERR_INVALID_ARGUMENT
    rows, q, codes = dd.small()
    ix = make_index(vdb, dd.EUCLID, rows)
    t = make_table(vdb, codes, dd.SM_N)

    def refused(res, what, code=E):
        rc, out = res
        assert rc == code, (what, rc, vdb._ffi.last_error())
        assert untouched(out), what

    refused(raw(vdb, ix, q, None, 4, 0, t, k=4), "g = 0")
    refused(raw(vdb, ix, q, None, 4, 33, t, k=4), "g = 33")
    refused(raw(vdb, ix, q, None, 1025, 2, t, k=1025), "k = 1025")
    refused(raw(vdb, ix, q, None, 4, 2, t, slot=3, k=4), "unknown slot")
    refused(raw(vdb, ix, q, None, 4, 2, None, k=4), "null table")
    refused(raw(vdb, ix, q, None, 4, 2, t, k=4, want_sizes=False), "null out_sizes")
    refused(raw(vdb, ix, q, None, 4, 2, t, k=4, want_ids=False), "null out_ids")
    refused(raw(vdb, ix, q, None, 3, 2, t, k=4), "kstride below k")
    for call in (lambda: ix.search_batch_per_group(q, 4, 0, t, 0), lambda: ix.search_batch_per_group(q, 4, 33, t, 0),
                 lambda: ix.search_batch_per_group(q, 1025, 2, t, 0), lambda: ix.search_batch_per_group(q, 4, 2, t, 9)):
        with pytest.raises(vdb.IndexError_):
            call()
    sh = make_index(vdb, dd.EUCLID, rows[:600], devices=[0, 0])
    refused(raw(vdb, sh, q, None, 4, 2, t, k=4), "sharded")
    assert "sharded" in vdb._ffi.last_error()[0]
    # k = 0 and an empty index: counts 0 before any other check (g = 0 and a null table included)
    rc, out = raw(vdb, ix, q, None, 1, 0, None, k=0)
    assert rc == 0 and (out[4] == 0).all() and (out[0] == POISON_ID).all() and (out[3] == POISON_S).all()
    empty = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    rc, out = raw(vdb, empty, q, None, 4, 0, None, k=4)
    assert rc == 0 and (out[4] == 0).all() and (out[3] == POISON_S).all() and empty.per_group_stats() == [dd.SM_NQ, 0, 0, 0, 0, 0, 0, 0]
    # the errors of the search by group come through: a query of another dimension
    with pytest.raises(vdb.DimensionMismatch):
        ix.search_batch_per_group(q[:, :5], 3, 2, t, 0)
    # ... and the call still answers
    ranks = [rd.ranking(("distinct small", b), dd.EUCLID, rows, q[b]) for b in range(dd.SM_NQ)]
    rc, out = raw(vdb, ix, q, None, 6, 4, t, k=6)
    assert rc == 0
    check(out, ranks, codes, 6, 4, "after the refusals")
    t.close()


def test_nan_row_inside_a_wanted_group(vdb):
    """a NaN row that is eligible only inside a wanted group fails the call; masked out, it is nobody's member"""
    rows, q, codes = pg.odd()
    rows = rows.copy()
    wanted = pg.expected(rd.ranking(("per group odd", 0), dd.EUCLID, rows, q[0]), codes, 3, 2)
    code = next(c for c, _, _ in wanted if c >= 0)
    ids = np.nonzero(codes == code)[0]
    ok = np.zeros(pg.ODD_N, dtype=bool)
    ok[ids] = True                                                             # the mask admits this one group ...
    bad = int(ids[-1])
    rows[bad, 7] = np.nan                                                      # ... one of whose rows has a NaN element
    ix = make_index(vdb, dd.EUCLID, rows)
    t = make_table(vdb, codes, pg.ODD_N)
    mask, bits = dd.id_mask(ok)
    with pytest.raises(vdb.NanDistance):
        ix.search_batch_per_group(q[:1], 3, 2, t, 0, id_mask=mask, mask_bits=bits)
    ok[bad] = False                                                            # masked out, it is nobody's member
    mask, bits = dd.id_mask(ok)
    got = ix.search_batch_per_group(q[:1], 3, 2, t, 0, id_mask=mask, mask_bits=bits)
    clean = pg.odd()[0]
    check(got, [rd.ranking(("per group odd one group", 0), dd.EUCLID, clean, q[0], live=ok.astype(np.uint8))], codes, 3, 2, "NaN row masked out")
    assert got[4][0] == 1 and got[3][0, 0] == 2
    t.close()


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [True, False])
def test_store_search_groups(vdb, device_filter):
    F = vdb.MetadataFilter
    n, d, k, g = 600, 16, 6, 3
    rng = np.random.default_rng(20274)
    rows = rng.standard_normal((n, d)).astype(F32)
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    doc = [None if i % 13 == 0 else f"doc-{(i * 7) % 40}" for i in range(n)]  # 40 documents; every 13th row has none
    lang = [("en", "de", "fr")[i % 3] for i in range(n)]
    st.set_device_filter(device_filter)
    half = n // 2
    for i in range(half):
        meta = {"lang": lang[i]}
        if doc[i] is not None:
            meta["doc"] = doc[i]
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata(meta))
    st.index().add_bulk(rows[half:], first_id=half)
    st.attach_bulk_metadata(n - half, {"doc": doc[half:], "lang": lang[half:]}, ids=[f"bulk-{i}" for i in range(half, n)])
    assert st.device_filter() == device_filter
    name = lambda i: f"item-{i}" if i < half else f"bulk-{i}"
    queries = [vdb.Vector((rows[i] + F32(0.01)).astype(F32)) for i in (3, 13, 299, 300, 599, 26, 77)]

    def restated(qv, ok):
        """the contract in numpy over the store's own metadata: [(value, [ids])]"""
        d2 = np.sqrt(((rows.astype(np.float64) - qv.data.astype(np.float64)) ** 2).sum(axis=1))
        order = [int(i) for i in np.lexsort((np.arange(n), d2)) if ok[i]]
        out, seen = [], set()
        for i in order:
            if doc[i] is None:
                out.append((None, [name(i)]))
            elif doc[i] not in seen:
                seen.add(doc[i])
                out.append((doc[i], [name(j) for j in order if doc[j] == doc[i]][:g]))
            if len(out) == k:
                break
        return out

    everyone = np.ones(n, dtype=bool)
    german = np.array([lang[i] == "de" for i in range(n)])
    for flt, ok in ((None, everyone), (F.Eq("lang", "de"), german)):
        got = st.search_groups_batch(queries, k, "doc", g, flt)
        for b, qv in enumerate(queries):
            assert [(v, [r.id for r in members]) for v, members in got[b]] == restated(qv, ok), (b, flt is not None)
        one = st.search_groups(queries[2], k, "doc", g, flt)
        assert [(v, [(r.id, r.distance) for r in m]) for v, m in one] == [(v, [(r.id, r.distance) for r in m]) for v, m in got[2]]
    # group_size 1 is search_distinct where that is available; a field nobody has is the plain search
    plain = st.search(queries[0], k)
    assert [(v, [(r.id, r.distance) for r in m]) for v, m in st.search_groups(queries[0], k, "nobody-has-this", g)] == \
        [(None, [(r.id, r.distance)]) for r in plain]
    if device_filter:
        ones = st.search_groups(queries[0], k, "doc", 1)
        assert [(m[0].id, m[0].distance) for _, m in ones] == [(r.id, r.distance) for r in st.search_distinct(queries[0], k, "doc")]
    with pytest.raises(ValueError):
        st.search_groups(queries[0], k, "doc", 0)
    with pytest.raises(ValueError):
        vdb.VectorStore(index=vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 40, 20), seed=1)).search_groups(queries[0], k, "doc", g)

"""Search by stored id (vdb_flat_search_batch_by_id, csrc/kernels_by_id.hip).  The contract is one sentence: for
query id x and count k the result is what vdb_flat_search_batch returns for the stored vector of x with k + 1 under the same mask,
the entry whose id equals x removed if it is there, cut to k.  Every case compares ids, order, distance bits and counts with that
expectation computed by the CPU oracle (tests/by_id_data.py; tests/test_by_id_cpu.py proves what the data is assumed to do)."""
import ctypes

import numpy as np
import pytest

import by_id_data as bd
import id_families
from conftest import load_package

pytestmark = pytest.mark.gpu

U64, F32 = np.uint64, np.float32
POISON_ID, POISON_D = U64(0xA5A5A5A5A5A5A5A5), np.uint32(0x7FC0BEEF)


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def make_index(vdb, metric, rows, ids=None, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(rows, ids=ids)
    return ix


def id_mask(ids, bits):
    ids = np.asarray(ids, dtype=U64)
    m = np.zeros((int(bits) + 63) // 64 + 1, dtype=U64)
    if ids.size:
        np.bitwise_or.at(m, (ids >> U64(6)).astype(np.int64), U64(1) << (ids & U64(63)))
    return m, int(bits)


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


_INDEX = {}


def scaled_index(vdb, metric):
    """the 20000 x 32 scaled-gaussian index of one metric, shared by the tests that do not change it"""
    if metric not in _INDEX:
        _INDEX[metric] = make_index(vdb, metric, bd.scaled())
    return _INDEX[metric]


# ------------------------------------------------------------------ three metrics, two routes
@pytest.mark.parametrize("metric", bd.METRICS)
def test_tiered_pipeline(vdb, metric):
    rows = bd.scaled()
    sel = bd.spaced(bd.N, 40)
    ix = scaled_index(vdb, metric)
    got = ix.search_batch_by_id(sel.astype(U64), bd.K)
    bd.check(got, bd.expected_cached("scaled40", metric, rows, sel, bd.K), "tiered")
    assert ix.by_id_stats()[0] == 40 and ix.by_id_stats()[3] == 0


@pytest.mark.parametrize("metric", bd.METRICS)
def test_direct_path_and_the_same_index_without_it(vdb, metric):
    rows = bd.scaled(300, 20)
    sel = np.array([0, 7, 150, 298, 299])
    want = bd.expected(metric, rows, sel, bd.K)
    ix = make_index(vdb, metric, rows)
    a = ix.search_batch_by_id(sel.astype(U64), bd.K)
    bd.check(a, want, "direct")
    ix.set_tiers(vdb.GpuFlatIndex.TIERS_NO_DIRECT)
    b = ix.search_batch_by_id(sel.astype(U64), bd.K)
    bd.check(b, want, "no direct")
    assert same(a, b)


def test_by_id_stats_split_under_dot(vdb):
    rows = bd.scaled()
    sel = bd.spaced(bd.N, bd.NSEL)
    want = bd.expected_cached("scaled96", bd.DOT, rows, sel, bd.K)
    ix = scaled_index(vdb, bd.DOT)
    bd.check(ix.search_batch_by_id(sel.astype(U64), bd.K), want, "dot 96")
    struck, cut = sum(1 for w in want if w[2]), sum(1 for w in want if w[3])
    assert struck > 0 and cut > 0
    assert ix.by_id_stats() == [bd.NSEL, struck, cut, 0]


@pytest.mark.parametrize("metric", [bd.EUCLID, bd.COSINE])
def test_triplicates_keep_the_twins(vdb, metric):
    rows, ids = bd.triplicates()
    sel = np.array([3 * v + c for v in (0, 5, 333, bd.TRI_V - 1) for c in (0, 1, 2)])
    want = bd.expected(metric, rows, sel, bd.K, ids=ids)
    ix = make_index(vdb, metric, rows, ids=ids)
    got = ix.search_batch_by_id(ids[sel], bd.K)
    bd.check(got, want, "triplicates")
    for b, r in enumerate(sel):
        twins = sorted(int(ids[r - r % 3 + c]) for c in range(3) if c != r % 3)
        assert got[0][b, :2].tolist() == twins and int(ids[r]) not in got[0][b].tolist(), (b, got[0][b])
    assert ix.by_id_stats() == [len(sel), len(sel), 0, 0]


@pytest.mark.parametrize("dim", [1, 33, 96])
def test_row_stride_differs_from_the_dimension(vdb, dim):
    """ld (the dimension rounded up to 32) differs from dim: the gather must honour the stride and copy no padding"""
    rows = bd.scaled(5000, dim)
    sel = np.array([0, 1, 31, 32, 33, 2500, 4097, 4998, 4999, 64, 65, 127])
    for metric in bd.METRICS:
        ix = make_index(vdb, metric, rows)
        bd.check(ix.search_batch_by_id(sel.astype(U64), bd.K), bd.expected(metric, rows, sel, bd.K), (dim, metric))


@pytest.mark.parametrize("nq", [1, 257, 600])
def test_batch_sizes(vdb, nq):
    """257 and 600 cross the 256- and 512-query passes; one id is asked about twice"""
    rows = bd.scaled()
    rng = np.random.default_rng(nq)
    sel = rng.choice(bd.N, nq, replace=False)
    if nq > 1:
        sel[nq - 1] = sel[0]
        sel[nq // 2] = sel[0]
    for metric in (bd.EUCLID, bd.DOT):
        ix = scaled_index(vdb, metric)
        got = ix.search_batch_by_id(sel.astype(U64), bd.K)
        bd.check(got, bd.expected(metric, rows, sel, bd.K), (nq, metric))
        assert ix.by_id_stats()[0] == nq
        if nq > 1:
            assert same([x[0] for x in got], [x[nq - 1] for x in got])


# ------------------------------------------------------------------ per-query ks
def raw_by_id(vdb, ix, qid, ks, kstride, k=0, width=None):
    """the C entry point itself, with poisoned outputs: ks an array (k unused) or None (k for every query)"""
    L = vdb._ffi.lib()
    qid = np.ascontiguousarray(qid, dtype=U64)
    nq = qid.size
    width = kstride if width is None else width
    oi = np.full((nq, width), POISON_ID, dtype=U64)
    od = np.full((nq, width), POISON_D, dtype=np.uint32).view(F32)
    oc = np.full(nq, 12345, dtype=np.uintp)
    u64p, szp, fp = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_float)
    ks_ptr = None
    if ks is not None:
        ks = np.ascontiguousarray(ks, dtype=np.uintp)
        ks_ptr = ks.ctypes.data_as(szp)
    rc = L.vdb_flat_search_batch_by_id(ix._h, qid.ctypes.data_as(u64p), nq, ks_ptr, k, None, 0, kstride,
                                       oi.ctypes.data_as(u64p), od.ctypes.data_as(fp), oc.ctypes.data_as(szp))
    return rc, oi, od, oc


@pytest.mark.parametrize("metric", bd.METRICS)
def test_per_query_ks_and_nothing_written_past_the_counts(vdb, metric):
    n = 600
    rows = bd.scaled(n, 8)
    sel = np.arange(0, n, 50)                                                  # 12 queries: not the direct path
    ks = np.array([0, 1, 10, n + 5] * 3)
    kstride = n + 5 + 3
    ix = make_index(vdb, metric, rows)
    rc, oi, od, oc = raw_by_id(vdb, ix, sel, ks, kstride)
    assert rc == 0, vdb._ffi.last_error()
    want = bd.expected(metric, rows, sel, ks)
    bd.check((oi, od, oc), want, "ks")
    for b in range(len(sel)):
        c = int(oc[b])
        assert c == min(int(ks[b]), n - 1), (b, c)                             # k = len + 5: everybody but the row itself
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(np.uint32) == POISON_D).all(), b
    # k = SIZE_MAX is clamped to len before the 1 is added: no wrap to k + 1 = 0
    size_max = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
    rc, oi, od, oc = raw_by_id(vdb, ix, sel[:1], None, size_max, k=size_max, width=n)
    assert rc == 0, vdb._ffi.last_error()
    bd.check((oi, od, oc), bd.expected(metric, rows, sel[:1], n + 5), "k = SIZE_MAX")
    assert int(oc[0]) == n - 1 and oi[0, n - 1] == POISON_ID


def test_k_112_enters_the_large_k_range(vdb):
    """k + 1 = 113 on 73200 rows: the first row count at which the large-k range serves 113"""
    L = vdb._ffi.lib()
    n = 73200
    assert L.vdb_flat_large_k_min_rows(113) == n and L.vdb_flat_large_k_min_rows(112) == 0
    rows = bd.scaled(n, 32)
    sel = bd.spaced(n, 12)
    ix = make_index(vdb, bd.EUCLID, rows)
    got = ix.search_batch_by_id(sel.astype(U64), 112)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1 and st["kprime"] > 112, st
    bd.check(got, bd.expected(bd.EUCLID, rows, sel, 112), "k 112")


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("every", [2, 100])
def test_masks_host_and_compiled(vdb, every):
    """50 % and 1 % selectivity; some query ids are eligible themselves, some are not -- those are still valid queries"""
    rows = bd.scaled()
    ok = (np.arange(bd.N) % every) == 0
    sel = np.concatenate([np.nonzero(ok)[0][[0, 3, 17, 50, 99]], np.nonzero(~ok)[0][[0, 1, 500, 5000, 9000]], [bd.N - 1, 2 * every]])
    assert ok[sel].any() and (~ok[sel]).any()
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, ok.astype(np.int32))
    table.set_present(0, bd.N, True)
    for metric in bd.METRICS:
        want = bd.expected(metric, rows, sel, bd.K, live=ok.astype(np.uint8))
        ix = scaled_index(vdb, metric)
        for sparse in (0, 1):
            ix.set_sparse_filter(sparse)
            a = ix.search_batch_by_id(sel.astype(U64), bd.K, id_mask=mask, mask_bits=bits)
            bd.check(a, want, (every, metric, sparse, "host mask"))
            assert ix.sparse_stats()[0] == sparse
            struck = sum(1 for w in want if w[2])
            assert ix.by_id_stats()[:2] == [len(sel), struck]
            if metric != bd.DOT:
                assert struck == int(ok[sel].sum())                                    # an eligible row finds itself, an ineligible one cannot
            with table.compile([(vdb.MetaTable.EQ, 0, 1)], bd.N) as cm:
                b = ix.search_batch_by_id(sel.astype(U64), bd.K, compiled_mask=cm)
            assert same(a, b), (every, metric, sparse)
        ix.set_sparse_filter(0)
    table.close()


# ------------------------------------------------------------------ mutations
def test_mutations(vdb):
    metric = bd.EUCLID
    n, d = 3000, 24
    rows = bd.scaled(n, d).copy()
    ids = np.arange(n, dtype=U64) * U64(3) + U64(1)
    live = np.ones(n, dtype=np.uint8)
    ix = make_index(vdb, metric, rows, ids=ids)
    sel = np.array([0, 10, 11, 999, 2000, 2999, 5, 6, 7, 8, 9, 12])
    bd.check(ix.search_batch_by_id(ids[sel], bd.K), bd.expected(metric, rows, sel, bd.K, ids=ids, live=live), "fresh")

    # an upserted id: the gather reads the NEW row (it is staged, not flushed, when the search arrives)
    new = (rows[10] * F32(-3.0) + F32(0.5)).astype(F32)
    ix.add(int(ids[10]), vdb.Vector(new))
    rows2 = np.concatenate([rows, new[None, :]])
    ids2 = np.concatenate([ids, ids[10:11]])
    live2 = np.concatenate([live, [1]]).astype(np.uint8)
    live2[10] = 0
    sel2 = np.array([0, n, 11, 999, 2000, 2999, 5, 6, 7, 8, 9, 12])           # device row n now carries id ids[10]
    want = bd.expected(metric, rows2, sel2, bd.K, ids=ids2, live=live2)
    bd.check(ix.search_batch_by_id(ids2[sel2], bd.K), want, "upsert")

    # an id added but not yet flushed
    extra = bd.scaled(n, d)[17] * F32(0.5)
    ix.add(10 ** 12, vdb.Vector(extra))
    rows3 = np.concatenate([rows2, extra[None, :]])
    ids3 = np.concatenate([ids2, [U64(10 ** 12)]])
    live3 = np.concatenate([live2, [1]]).astype(np.uint8)
    sel3 = np.concatenate([sel2, [n + 1]])
    bd.check(ix.search_batch_by_id(ids3[sel3], bd.K), bd.expected(metric, rows3, sel3, bd.K, ids=ids3, live=live3), "staged add")

    # a removed id fails the whole batch and is named; nothing is searched
    ix.remove(int(ids[999]))
    live3[999] = 0
    with pytest.raises(vdb.VectorNotFound) as e:
        ix.search_batch_by_id(ids3[sel3], bd.K)
    assert e.value.id == int(ids[999])
    rc, _, _, oc = raw_by_id(vdb, ix, ids3[sel3], np.full(len(sel3), 3), 4)
    assert rc == vdb._ffi.ERR_NOT_FOUND and str(int(ids[999])) in vdb._ffi.last_error()[0] and (oc == 12345).all()
    with pytest.raises(vdb.VectorNotFound) as e:
        ix.search_batch_by_id(np.array([ids[0], 2, ids[999]], dtype=U64), bd.K)      # 2 was never added: the FIRST absent id is named
    assert e.value.id == 2
    sel4 = sel3[sel3 != 999]
    bd.check(ix.search_batch_by_id(ids3[sel4], bd.K), bd.expected(metric, rows3, sel4, bd.K, ids=ids3, live=live3), "after remove")

    # after compact(): rows moved, ids did not
    for r in range(100, 1100, 2):
        if live3[r]:
            ix.remove(int(ids3[r]))
            live3[r] = 0
    sel5 = np.array([r for r in sel4 if live3[r]] + [101, 1099, 1101])
    want5 = bd.expected(metric, rows3, sel5, bd.K, ids=ids3, live=live3)
    before = ix.search_batch_by_id(ids3[sel5], bd.K)
    assert ix.compact() > 0
    after = ix.search_batch_by_id(ids3[sel5], bd.K)
    bd.check(before, want5, "before compact")
    bd.check(after, want5, "after compact")

    # a row of another dimension: the error of searching with that vector
    odd = np.ones(d + 3, dtype=F32)
    ix.add(777, vdb.Vector(odd))
    with pytest.raises(vdb.DimensionMismatch) as e1:
        ix.search_batch_arrays(odd[None, :], bd.K)
    with pytest.raises(vdb.DimensionMismatch) as e2:
        ix.search_batch_by_id(np.array([777], dtype=U64), bd.K)
    assert (e2.value.expected, e2.value.actual) == (e1.value.expected, e1.value.actual) == (d + 3, d)
    with pytest.raises(vdb.DimensionMismatch) as e3:                                   # ... and a fitting query id fails as its search does
        ix.search_batch_by_id(ids3[sel5[:2]], bd.K)
    with pytest.raises(vdb.DimensionMismatch) as e4:
        ix.search_batch_arrays(rows3[sel5[:2]], bd.K)
    assert (e3.value.expected, e3.value.actual) == (e4.value.expected, e4.value.actual) == (d, d + 3)
    ix.remove(777)
    bd.check(ix.search_batch_by_id(ids3[sel5], bd.K), want5, "misfit removed")


def test_empty_batch_and_empty_index(vdb):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    gi, gd, gc = ix.search_batch_by_id(np.zeros(0, dtype=U64), 5)
    assert gc.size == 0 and ix.by_id_stats() == [0, 0, 0, 0]
    with pytest.raises(vdb.VectorNotFound):
        ix.search_batch_by_id(np.array([0], dtype=U64), 5)
    ix.add(4, vdb.Vector(np.ones(3, dtype=F32)))
    gi, gd, gc = ix.search_batch_by_id(np.array([4, 4], dtype=U64), 5)                 # alone in the index: nothing is near it
    assert gc.tolist() == [0, 0] and ix.by_id_stats() == [2, 2, 0, 0]


# ------------------------------------------------------------------ id space
@pytest.mark.parametrize("family", ["across32", "across63", "top", "high_word_only", "low_word_only"])
def test_id_space(vdb, family):
    """the strike compares all 64 bits and treats no value as a flag: 2^64 - 1 is a stored id and a query id"""
    n, d = 2000, 16
    rows = bd.scaled(n, d)
    labels = id_families.permutation(n)
    ids = id_families.family_ids(family, n, labels)
    last = int(np.argmax(ids))                                                 # the row with the largest id of the family
    sel = np.array([0, 1, last, n - 1, 500, 501, 502, 503, 504, 505, 506, 507])
    if family == "top":
        assert int(ids[last]) == 2 ** 64 - 1
    for metric in bd.METRICS:
        ix = make_index(vdb, metric, rows, ids=ids)
        want = bd.expected(metric, rows, sel, bd.K, ids=ids)
        bd.check(ix.search_batch_by_id(ids[sel], bd.K), want, (family, metric))
        assert ix.by_id_stats() == [len(sel), sum(1 for w in want if w[2]), sum(1 for w in want if w[3]), 0]
        bd.check(ix.search_batch_by_id(ids[sel[:3]], bd.K), want[:3], (family, metric, "direct"))


# ------------------------------------------------------------------ errors of the equivalent search
def test_cosine_errors(vdb):
    n, d = 2000, 16
    rows = bd.scaled(n, d).copy()
    ix = make_index(vdb, bd.COSINE, rows)
    ix.add(n, vdb.Vector(np.zeros(d, dtype=F32)))
    for q in ([5], [n], list(range(12))):                                      # a zero-norm row fails every search, whoever asks
        with pytest.raises(vdb.InvalidVector):
            ix.search_batch_by_id(np.array(q, dtype=U64), bd.K)
    ix.remove(n)
    bd.check(ix.search_batch_by_id(np.arange(12, dtype=U64), bd.K), bd.expected(bd.COSINE, rows, np.arange(12), bd.K), "zero row removed")
    bad = rows[3].copy()
    bad[2] = np.nan
    ix.add(n + 1, vdb.Vector(bad))
    for q in ([n + 1], [n + 1] + list(range(11))):
        with pytest.raises(vdb.NanDistance):
            ix.search_batch_by_id(np.array(q, dtype=U64), bd.K)


# ------------------------------------------------------------------ sharded handle
@pytest.mark.parametrize("metric", bd.METRICS)
def test_sharded_handle(vdb, metric):
    rows = bd.scaled()
    sh = make_index(vdb, metric, rows, devices=[0, 0, 0])
    assert sh.shards() == 3 and all(sh.shard_len(g) > 0 for g in range(3))
    bounds = np.cumsum([0] + [sh.shard_len(g) for g in range(3)])
    sel = np.array([0, 1, bounds[1] - 1, bounds[1], bounds[1] + 7, bounds[2] - 1, bounds[2], bd.N - 1, 3, bounds[2] + 100, bounds[1] + 2, 5, 0])
    assert all(((sel >= bounds[g]) & (sel < bounds[g + 1])).any() for g in range(3))   # query ids from all three shards
    want = bd.expected(metric, rows, sel, bd.K)
    got = sh.search_batch_by_id(sel.astype(U64), bd.K)
    bd.check(got, want, "sharded")
    assert sh.by_id_stats() == [len(sel), sum(1 for w in want if w[2]), sum(1 for w in want if w[3]), 0]
    assert same(got, scaled_index(vdb, metric).search_batch_by_id(sel.astype(U64), bd.K))
    # under a mask, with per-query ks
    ok = (np.arange(bd.N) % 3) != 1
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    ks = np.array([0, 1, 10, 7] * 3 + [10])
    bd.check(sh.search_batch_by_id(sel.astype(U64), ks, id_mask=mask, mask_bits=bits),
             bd.expected(metric, rows, sel, ks, live=ok.astype(np.uint8)), "sharded, masked")
    # an id on no shard; a staged single add on some shard
    with pytest.raises(vdb.VectorNotFound) as e:
        sh.search_batch_by_id(np.array([1, bd.N + 5], dtype=U64), bd.K)
    assert e.value.id == bd.N + 5
    extra = (rows[9] * F32(1.5)).astype(F32)
    sh.add(bd.N + 5, vdb.Vector(extra))
    rows2 = np.concatenate([rows, extra[None, :]])
    ids2 = np.concatenate([np.arange(bd.N, dtype=U64), [U64(bd.N + 5)]])
    sel2 = np.array([bd.N, 9, bounds[1], bounds[2]] + list(range(20, 28)))
    bd.check(sh.search_batch_by_id(ids2[sel2], bd.K), bd.expected(metric, rows2, sel2, bd.K, ids=ids2), "sharded, staged add")


# ------------------------------------------------------------------ tickets
def test_refused_while_a_ticket_is_outstanding(vdb):
    import torch
    rows = bd.scaled()
    ix = make_index(vdb, bd.EUCLID, rows)                                      # (its own handle: a ticket blocks every other caller)
    dev = torch.device("cuda", 0)
    B = 16
    q = torch.from_numpy(rows[:B].copy()).to(dev)
    out = (torch.empty((B, bd.K), dtype=torch.int64, device=dev), torch.empty((B, bd.K), dtype=torch.float32, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev))
    sel = bd.spaced(bd.N, 40)
    t = ix.search_batch_device_submit(q.data_ptr(), B, bd.D, bd.K, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    try:
        with pytest.raises(vdb.VectorDbError):
            ix.search_batch_by_id(sel.astype(U64), bd.K)
    finally:
        ix.search_batch_device_wait(t)
    torch.cuda.synchronize()
    bd.check(ix.search_batch_by_id(sel.astype(U64), bd.K), bd.expected_cached("scaled40", bd.EUCLID, rows, sel, bd.K), "after the ticket")


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_search_similar(vdb, device_filter):
    F = vdb.MetadataFilter
    n, d, k = 400, 12, 6
    rows = bd.scaled(n, d)
    st = vdb.VectorStore(vdb.DistanceMetric.DotProduct)
    if device_filter:
        st.set_device_filter(True)
    half = n // 2
    for i in range(half):                                                      # inserted rows: string ids, metadata objects
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata({"color": ("blue", "green", "red")[i % 3]}))
    st.index().add_bulk(rows[half:], first_id=half)                             # bulk-attached rows: ids of their own
    st.attach_bulk_metadata(n - half, {"color": [("blue", "green", "red")[i % 3] for i in range(half, n)]},
                            ids=[f"bulk-{i}" for i in range(half, n)])
    assert st.device_filter() == device_filter
    name = lambda i: f"item-{i}" if i < half else f"bulk-{i}"
    sel = np.array([0, 1, 2, 5, half - 1, half, half + 1, n - 1, 100, 301, 302, 303])
    red = (np.arange(n) % 3) == 2                                              # the large rows: under Dot they find themselves
    for flt, live in ((None, None), (F.Eq("color", "red"), red.astype(np.uint8))):
        want = bd.expected(bd.DOT, rows, sel, k, live=live)
        got = st.search_similar_batch([name(i) for i in sel], k, flt)
        assert len(got) == len(sel)
        for b, (oi, od, _, _) in enumerate(want):
            assert [r.id for r in got[b]] == [name(int(i)) for i in oi], (b, flt is not None)
            assert np.array_equal(np.array([r.distance for r in got[b]], dtype=F32).view(np.uint32), od.view(np.uint32)), b
        one = st.search_similar(name(int(sel[3])), k, flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[3]]
    assert any(w[2] for w in want) and any(w[3] for w in want)                  # red and non-red query ids
    with pytest.raises(vdb.VectorNotFound):
        st.search_similar("nobody", k)
    with pytest.raises(vdb.VectorNotFound):
        st.search_similar_batch([name(0), "bulk-3"], k)                        # 3 is an inserted row: no bulk id names it
    st.delete(name(5))
    with pytest.raises(vdb.VectorNotFound):
        st.search_similar(name(5), k)

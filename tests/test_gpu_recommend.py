"""Recommend from positive and negative stored ids (vdb_flat_recommend_batch, csrc/kernels_recommend.hip).  The
contract is one sentence: for request b the result is what vdb_flat_search_batch returns for the fold q_b of its examples with
k_b + m_b under the same mask, every entry whose id is among the examples removed, cut to k_b.  Every case compares every request
-- ids, order, distance bits and counts -- with that expectation computed by the CPU oracle over the numpy restatement of the
fold (tests/recommend_data.py; tests/test_recommend_cpu.py proves that the data makes a wrong fold order, a division or a wrong
strike visible)."""
import ctypes

import numpy as np
import pytest

import by_id_data as bd
import recommend_data as rd
from conftest import load_package

pytestmark = pytest.mark.gpu

U64, F32 = np.uint64, np.float32
POISON_ID, POISON_D = U64(0xA5A5A5A5A5A5A5A5), np.uint32(0x7FC0BEEF)
TOP = 2 ** 64 - 1


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


def recommend(ix, reqs, k, ids=None, **kw):
    pos, neg = rd.split(reqs, ids)
    return ix.recommend_batch(pos, neg, k, **kw)


_INDEX = {}


def scaled_index(vdb, metric):
    """the 20000 x 32 scaled-gaussian index of one metric, shared by the tests that do not change it"""
    if metric not in _INDEX:
        _INDEX[metric] = make_index(vdb, metric, bd.scaled())
    return _INDEX[metric]


# ------------------------------------------------------------------ the fold
@pytest.mark.parametrize("metric", rd.METRICS)
@pytest.mark.parametrize("dim", [33, 64, 1100])
def test_fold_shapes(vdb, dim, metric):
    """dim 33: the scalar path, ld = 64 differs from dim; 64: the 16-byte path; 1100: two workgroups along the row.  One batch
    holds m = 1, 2, 5, 9 and 64, requests with and without negatives, an id listed twice and an id on both sides."""
    rows = rd.fold_rows(dim)
    reqs = rd.fold_requests()
    ix = make_index(vdb, metric, rows)
    got = recommend(ix, reqs, rd.K)
    rd.check(got, rd.expected(metric, rows, reqs, rd.K), (dim, metric))
    assert ix.recommend_stats() == rd.stats(metric, rows, reqs, rd.K, rd.FOLD_N)
    assert ix.recommend_stats()[3] == rd.K + 64


@pytest.mark.parametrize("metric", rd.METRICS)
def test_tiered_pipeline_and_both_strike_outcomes(vdb, metric):
    rows = bd.scaled()
    reqs = rd.scaled_requests()
    ix = scaled_index(vdb, metric)
    got = recommend(ix, reqs, rd.K)
    rd.check(got, rd.expected_cached("scaled24", metric, rows, reqs, rd.K), "scaled")
    st = rd.stats(metric, rows, reqs, rd.K, bd.N)
    assert ix.recommend_stats() == st
    if metric == rd.DOT:
        assert 0 < st[2] < st[1]                                               # some examples were in their list, some were not


@pytest.mark.parametrize("metric", rd.METRICS)
def test_one_positive_is_search_by_id_bit_for_bit(vdb, metric):
    rows = bd.scaled()
    sel = bd.spaced(bd.N, bd.NSEL)
    ix = scaled_index(vdb, metric)
    reqs = [((int(r),), ()) for r in sel]
    a = recommend(ix, reqs, bd.K)
    b = ix.search_batch_by_id(sel.astype(U64), bd.K)
    assert same(a, b)
    bd.check(a, bd.expected_cached("scaled96", metric, rows, sel, bd.K), "identity")
    ok = (np.arange(bd.N) % 2) == 0
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    a = recommend(ix, reqs, bd.K, id_mask=mask, mask_bits=bits)
    b = ix.search_batch_by_id(sel.astype(U64), bd.K, id_mask=mask, mask_bits=bits)
    assert same(a, b)
    rd.check(a, rd.expected(metric, rows, reqs, bd.K, live=ok.astype(np.uint8)), "identity, masked")


# ------------------------------------------------------------------ the strike
@pytest.mark.parametrize("metric", [rd.EUCLID, rd.COSINE])
def test_triplicates(vdb, metric):
    """all three copies of a vector as examples; one copy, so that its twins precede and follow the neighbours; a copy on each side"""
    rows, ids = bd.triplicates()
    t = rd.tri_row
    reqs = [((t(5, 0), t(5, 1), t(5, 2)), ()), ((t(9, 1),), ()), ((t(20, 0),), (t(20, 2),)), ((t(9, 0), t(9, 2)), ()),
            ((t(333, 2), t(5, 1)), (t(699, 0),)), ((t(0, 0),), ()), ((t(699, 2),), ()), ((t(1, 1), t(1, 1)), ()), ((t(2, 0),), (t(3, 0), t(3, 1)))]
    ix = make_index(vdb, metric, rows, ids=ids)
    got = recommend(ix, reqs, rd.K, ids=ids)
    rd.check(got, rd.expected(metric, rows, reqs, rd.K, ids=ids), "triplicates")
    assert ix.recommend_stats() == rd.stats(metric, rows, reqs, rd.K, len(rows), ids=ids)
    assert not np.isin(got[0][0], ids[[t(5, 0), t(5, 1), t(5, 2)]]).any()
    assert got[0][1, :2].tolist() == sorted(int(ids[t(9, c)]) for c in (0, 2))    # the twins of the single example lead its list
    assert got[0][2, 0] == ids[t(20, 1)]


def test_list_of_two_chunks_and_a_masked_example(vdb):
    """k = 250, m = 20: the 270-entry list spans two chunks of the compaction, with examples in front of position 255 and behind
    256; then the same under a mask that makes three examples and every fifth row ineligible"""
    rows, ids = bd.triplicates()
    straddle = rd.tri_straddle()
    t = rd.tri_row
    reqs = [straddle, ((t(5, 0), t(5, 1), t(5, 2)), ()), (straddle[0][:7], straddle[0][7:])]
    ix = make_index(vdb, rd.EUCLID, rows, ids=ids)
    got = recommend(ix, reqs, rd.TRI_K, ids=ids)
    rd.check(got, rd.expected(rd.EUCLID, rows, reqs, rd.TRI_K, ids=ids), "two chunks")
    st = rd.stats(rd.EUCLID, rows, reqs, rd.TRI_K, len(rows), ids=ids)
    assert ix.recommend_stats() == st and st[3] == rd.TRI_K + rd.TRI_M and st[2] >= 6
    live = (np.arange(len(rows)) % 5 != 4).astype(np.uint8)
    live[list(straddle[0][:3])] = 0
    mask, bits = id_mask(ids[np.nonzero(live)[0]], 3 * bd.TRI_V)
    got = recommend(ix, reqs, rd.TRI_K, ids=ids, id_mask=mask, mask_bits=bits)
    rd.check(got, rd.expected(rd.EUCLID, rows, reqs, rd.TRI_K, ids=ids, live=live), "two chunks, masked")
    assert ix.recommend_stats() == rd.stats(rd.EUCLID, rows, reqs, rd.TRI_K, len(rows), ids=ids, live=live)


def raw_recommend(vdb, ix, ex, offsets, n_pos, ks, kstride, k=0, width=None, nq=None):
    """the C entry point itself, with poisoned outputs: ks an array (k unused) or None (k for every request); any of ex / offsets /
    n_pos may be None (a null pointer)"""
    L = vdb._ffi.lib()
    u64p, szp, fp, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float, ctypes.c_uint32))
    ex = None if ex is None else np.ascontiguousarray(ex, dtype=U64)
    offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uintp)
    n_pos = None if n_pos is None else np.ascontiguousarray(n_pos, dtype=np.uint32)
    nq = (len(offsets) - 1 if offsets is not None else len(n_pos)) if nq is None else nq
    width = kstride if width is None else width
    oi = np.full((nq, width), POISON_ID, dtype=U64)
    od = np.full((nq, width), POISON_D, dtype=np.uint32).view(F32)
    oc = np.full(nq, 12345, dtype=np.uintp)
    ks_ptr = None
    if ks is not None:
        ks = np.ascontiguousarray(ks, dtype=np.uintp)
        ks_ptr = ks.ctypes.data_as(szp)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    rc = L.vdb_flat_recommend_batch(ix._h, ptr(ex, u64p), ptr(offsets, szp), ptr(n_pos, u32p), nq, ks_ptr, k, None, 0, kstride,
                                    oi.ctypes.data_as(u64p), od.ctypes.data_as(fp), oc.ctypes.data_as(szp))
    return rc, oi, od, oc


@pytest.mark.parametrize("metric", rd.METRICS)
def test_per_request_ks_counts_and_nothing_written_past_them(vdb, metric):
    """one search at depth min(max ks, len) + 4 = len, one strike, a prefix per request; k >= len leaves everybody but the examples"""
    n = 64
    rows = bd.scaled(n, 8)
    req = ((3, 7, 9), (11,))
    ks = [0, 1, 60, 61, 64, 500, 10, 2, 59, 60, 3, 1]
    reqs = [req] * len(ks)
    ix = make_index(vdb, metric, rows)
    ex = np.array(list(req[0] + req[1]) * len(ks))
    offsets = np.arange(len(ks) + 1) * 4
    rc, oi, od, oc = raw_recommend(vdb, ix, ex, offsets, [3] * len(ks), ks, 503)
    assert rc == 0, vdb._ffi.last_error()
    rd.check((oi, od, oc), rd.expected(metric, rows, reqs, ks), "ks")
    for b, kb in enumerate(ks):
        c = int(oc[b])
        assert c == min(kb, n - 4), (b, c)
        assert (oi[b, c:] == POISON_ID).all() and (od[b, c:].view(np.uint32) == POISON_D).all(), b
    assert ix.recommend_stats() == [len(ks), 4 * len(ks), 4 * len(ks), n]
    # k = SIZE_MAX is clamped to len before m is added: no wrap
    size_max = 2 ** (8 * ctypes.sizeof(ctypes.c_size_t)) - 1
    rc, oi, od, oc = raw_recommend(vdb, ix, ex[:4], [0, 4], [3], None, size_max, k=size_max, width=n)
    assert rc == 0, vdb._ffi.last_error()
    rd.check((oi, od, oc), rd.expected(metric, rows, [req], n + 5), "k = SIZE_MAX")
    assert int(oc[0]) == n - 4 and oi[0, n - 4] == POISON_ID


def test_len_at_most_m_leaves_nobody(vdb):
    rows = bd.scaled(4, 8)
    ix = make_index(vdb, rd.EUCLID, rows)
    gi, gd, gc = ix.recommend_batch([[0, 1], [2], [3, 3, 3, 3, 3]], [[2, 3], [], []], 5)
    reqs = [((0, 1), (2, 3)), ((2,), ()), ((3, 3, 3, 3, 3), ())]
    rd.check((gi, gd, gc), rd.expected(rd.EUCLID, rows, reqs, 5), "tiny")
    assert gc.tolist() == [0, 3, 3] and ix.recommend_stats() == [3, 10, 6, 4]


def test_empty_batch_and_empty_index(vdb):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    gi, gd, gc = ix.recommend_batch([], [], 5)
    assert gc.size == 0 and ix.recommend_stats() == [0, 0, 0, 0]
    with pytest.raises(vdb.VectorNotFound):
        ix.recommend_batch([[0]], [[]], 5)
    ix.add(4, vdb.Vector(np.ones(3, dtype=F32)))
    gi, gd, gc = ix.recommend_batch([[4], [4, 4]], None, 5)                    # alone in the index: nothing is near it
    assert gc.tolist() == [0, 0] and ix.recommend_stats() == [2, 3, 2, 1]


def test_id_2_to_the_64_minus_1_is_an_example_and_a_neighbour(vdb):
    rows, ids = bd.triplicates()
    ids = ids.copy()
    t = rd.tri_row
    ids[t(7, 2)] = U64(TOP)
    reqs = [((t(7, 2),), ()), ((t(7, 0),), ()), ((t(7, 0), t(7, 2)), ()), ((t(8, 1),), (t(7, 2),)), ((t(7, 1),), (t(7, 1),))]
    for metric in (rd.EUCLID, rd.DOT):
        ix = make_index(vdb, metric, rows, ids=ids)
        got = recommend(ix, reqs, rd.K, ids=ids)
        rd.check(got, rd.expected(metric, rows, reqs, rd.K, ids=ids), ("top", metric))
        assert ix.recommend_stats() == rd.stats(metric, rows, reqs, rd.K, len(rows), ids=ids)
        if metric == rd.EUCLID:
            assert TOP not in got[0][0].tolist() and TOP in got[0][1, :2].tolist() and TOP not in got[0][2].tolist()


# ------------------------------------------------------------------ tier edges
def test_k_plus_m_crosses_112(vdb):
    """k = 100, m = 13: the search runs with 113 on 73200 rows, the first row count at which the large-k range serves 113"""
    L = vdb._ffi.lib()
    n = 73200
    assert L.vdb_flat_large_k_min_rows(113) <= n
    rows = bd.scaled(n, 32)
    rng = np.random.default_rng(20273)
    reqs = []
    for _ in range(12):
        e = [int(x) for x in rng.choice(n, 13, replace=False)]
        reqs.append((tuple(e[:8]), tuple(e[8:])))
    ix = make_index(vdb, rd.EUCLID, rows)
    got = recommend(ix, reqs, 100)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1 and st["kprime"] > 112, st
    rd.check(got, rd.expected(rd.EUCLID, rows, reqs, 100), "k 100 + 13")
    assert ix.recommend_stats()[3] == 113


@pytest.mark.parametrize("metric", [rd.EUCLID, rd.DOT])
def test_forced_tiers_give_the_same_bits(vdb, metric):
    rows = bd.scaled()
    reqs = rd.scaled_requests()
    want = rd.expected_cached("scaled24", metric, rows, reqs, rd.K)
    ix = scaled_index(vdb, metric)
    G = vdb.GpuFlatIndex
    try:
        base = recommend(ix, reqs, rd.K)
        for flags in (G.TIERS_NO_DIRECT, G.TIERS_FORCE_F32, G.TIERS_FORCE_EXACT):
            ix.set_tiers(flags)
            got = recommend(ix, reqs, rd.K)
            rd.check(got, want, (metric, flags))
            assert same(got, base), flags
    finally:
        ix.set_tiers(0)
    small = rd.fold_rows(64)
    few = rd.fold_requests()[:5]                                               # a batch the direct path would take: it is bypassed
    sx = make_index(vdb, metric, small)
    a = recommend(sx, few, rd.K)
    sx.set_tiers(G.TIERS_NO_DIRECT)
    assert same(a, recommend(sx, few, rd.K))
    rd.check(a, rd.expected(metric, small, few, rd.K), "small")


# ------------------------------------------------------------------ masks
@pytest.mark.parametrize("every", [2, 100])
def test_masks_host_and_compiled(vdb, every):
    """50 % and 1 % selectivity; some examples are eligible themselves, some are not -- those are still valid examples"""
    rows = bd.scaled()
    ok = (np.arange(bd.N) % every) == 0
    reqs = rd.scaled_requests()
    flat = np.array([e for p, n in reqs for e in p + n])
    assert ok[flat].any() and (~ok[flat]).any()
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, ok.astype(np.int32))
    table.set_present(0, bd.N, True)
    for metric in rd.METRICS:
        want = rd.expected(metric, rows, reqs, rd.K, live=ok.astype(np.uint8))
        ix = scaled_index(vdb, metric)
        for sparse in (0, 1):
            ix.set_sparse_filter(sparse)
            a = recommend(ix, reqs, rd.K, id_mask=mask, mask_bits=bits)
            rd.check(a, want, (every, metric, sparse, "host mask"))
            assert ix.sparse_stats()[0] == sparse
            with table.compile([(vdb.MetaTable.EQ, 0, 1)], bd.N) as cm:
                b = recommend(ix, reqs, rd.K, compiled_mask=cm)
            assert same(a, b), (every, metric, sparse)
        ix.set_sparse_filter(0)
    table.close()


# ------------------------------------------------------------------ sharded handle
@pytest.mark.parametrize("metric", rd.METRICS)
def test_sharded_handle(vdb, metric):
    rows = bd.scaled()
    sh = make_index(vdb, metric, rows, devices=[0, 0, 0])
    assert sh.shards() == 3 and all(sh.shard_len(g) > 0 for g in range(3))
    bounds = np.cumsum([0] + [sh.shard_len(g) for g in range(3)])
    b1, b2 = int(bounds[1]), int(bounds[2])
    # every request's examples lie on three shards, in an order that is not the shards' order
    reqs = [((b2 + 5, 2, b1 + 2), ()), ((b1, 0, b2), (bd.N - 1, 1)), ((b2 - 1, b1 - 1, bd.N - 2, 5, b1 + 8), (b2 + 1, 3, b1 + 9, 7)),
            ((4,), ()), ((b1 + 4, b1 + 4, 8), (b2 + 8,)), ((b2 + 2, 11), (11, b1 + 11))] + list(rd.scaled_requests()[:8])
    for p, n in reqs[:3]:
        assert all(((np.array(p + n) >= bounds[g]) & (np.array(p + n) < bounds[g + 1])).any() for g in range(3))
    want = rd.expected(metric, rows, reqs, rd.K)
    got = recommend(sh, reqs, rd.K)
    rd.check(got, want, "sharded")
    assert sh.recommend_stats() == rd.stats(metric, rows, reqs, rd.K, bd.N)
    assert same(got, recommend(scaled_index(vdb, metric), reqs, rd.K))
    # under a mask, with per-request ks
    ok = (np.arange(bd.N) % 3) != 1
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    ks = np.array([0, 1, 10, 7] * 3 + [10, 2])
    rd.check(recommend(sh, reqs, ks, id_mask=mask, mask_bits=bits), rd.expected(metric, rows, reqs, ks, live=ok.astype(np.uint8)), "sharded, masked")
    # an id on no shard; a staged single add on some shard
    with pytest.raises(vdb.VectorNotFound) as e:
        sh.recommend_batch([[1, bd.N + 5]], [[2]], rd.K)
    assert e.value.id == bd.N + 5
    extra = (rows[9] * F32(1.5)).astype(F32)
    sh.add(bd.N + 5, vdb.Vector(extra))
    rows2 = np.concatenate([rows, extra[None, :]])
    ids2 = np.concatenate([np.arange(bd.N, dtype=U64), [U64(bd.N + 5)]])
    reqs2 = [((bd.N, b1, b2 + 3), (9,)), ((b1 + 1, bd.N), ())] + reqs[:10]
    rd.check(recommend(sh, reqs2, rd.K, ids=ids2), rd.expected(metric, rows2, reqs2, rd.K, ids=ids2), "sharded, staged add")


# ------------------------------------------------------------------ state
def test_mutations(vdb):
    metric = rd.EUCLID
    n, d = 3000, 24
    rows = bd.scaled(n, d).copy()
    ids = np.arange(n, dtype=U64) * U64(3) + U64(1)
    live = np.ones(n, dtype=np.uint8)
    ix = make_index(vdb, metric, rows, ids=ids)
    reqs = [((0, 10, 11), (999,)), ((2000,), ()), ((2999, 5, 6, 7, 8), (9, 12, 10)), ((10,), (11,)), ((20, 21), ()), ((30,), (31, 32)),
            ((40, 41, 42, 43), ()), ((50,), ()), ((60, 61), (62,)), ((70,), ()), ((80, 81, 82), ()), ((90,), (91,))]
    rd.check(recommend(ix, reqs, rd.K, ids=ids), rd.expected(metric, rows, reqs, rd.K, ids=ids, live=live), "fresh")

    # a re-added id: the fold reads the NEW row (it is staged, not flushed, when the call arrives)
    new = (rows[10] * F32(-3.0) + F32(0.5)).astype(F32)
    ix.add(int(ids[10]), vdb.Vector(new))
    rows2 = np.concatenate([rows, new[None, :]])
    ids2 = np.concatenate([ids, ids[10:11]])
    live2 = np.concatenate([live, [1]]).astype(np.uint8)
    live2[10] = 0
    swap = lambda t: tuple(n if r == 10 else r for r in t)                     # device row n now carries id ids[10]
    reqs2 = [(swap(p), swap(q)) for p, q in reqs]
    want2 = rd.expected(metric, rows2, reqs2, rd.K, ids=ids2, live=live2)
    got2 = recommend(ix, reqs2, rd.K, ids=ids2)
    rd.check(got2, want2, "re-added")
    assert not same(got2, recommend(make_index(vdb, metric, rows, ids=ids), reqs, rd.K, ids=ids))

    # an id added but not yet flushed is seen, as an example and as a neighbour
    extra = (rows[17] * F32(0.5)).astype(F32)
    ix.add(10 ** 12, vdb.Vector(extra))
    rows3 = np.concatenate([rows2, extra[None, :]])
    ids3 = np.concatenate([ids2, [U64(10 ** 12)]])
    live3 = np.concatenate([live2, [1]]).astype(np.uint8)
    reqs3 = reqs2 + [((n + 1, 17), ()), ((17,), ())]
    rd.check(recommend(ix, reqs3, rd.K, ids=ids3), rd.expected(metric, rows3, reqs3, rd.K, ids=ids3, live=live3), "staged add")

    # a removed example fails the whole batch and is named; nothing is searched
    ix.remove(int(ids[999]))
    live3[999] = 0
    with pytest.raises(vdb.VectorNotFound) as e:
        recommend(ix, reqs3, rd.K, ids=ids3)
    assert e.value.id == int(ids[999])
    reqs4 = [((0, n, 11), ())] + reqs3[1:]
    rd.check(recommend(ix, reqs4, rd.K, ids=ids3), rd.expected(metric, rows3, reqs4, rd.K, ids=ids3, live=live3), "after remove")

    # after compact(): rows moved, ids did not
    for r in range(100, 1100, 2):
        if live3[r]:
            ix.remove(int(ids3[r]))
            live3[r] = 0
    reqs5 = reqs4 + [((101, 1099, 1101), (2500,))]
    want5 = rd.expected(metric, rows3, reqs5, rd.K, ids=ids3, live=live3)
    before = recommend(ix, reqs5, rd.K, ids=ids3)
    assert ix.compact() > 0
    after = recommend(ix, reqs5, rd.K, ids=ids3)
    rd.check(before, want5, "before compact")
    rd.check(after, want5, "after compact")
    assert same(before, after)

    # a row of another dimension: the error of searching with that vector
    odd = np.ones(d + 3, dtype=F32)
    ix.add(777, vdb.Vector(odd))
    with pytest.raises(vdb.DimensionMismatch) as e1:
        ix.search_batch_arrays(odd[None, :], rd.K)
    with pytest.raises(vdb.DimensionMismatch) as e2:
        ix.recommend_batch([[777, int(ids3[0])]], [[]], rd.K)
    assert (e2.value.expected, e2.value.actual) == (e1.value.expected, e1.value.actual) == (d + 3, d)
    with pytest.raises(vdb.DimensionMismatch) as e3:                                   # ... and fitting examples fail as their search does
        recommend(ix, reqs5[:2], rd.K, ids=ids3)
    with pytest.raises(vdb.DimensionMismatch) as e4:
        ix.search_batch_arrays(rd.queries(rows3, reqs5[:2]), rd.K)
    assert (e3.value.expected, e3.value.actual) == (e4.value.expected, e4.value.actual) == (d, d + 3)
    ix.remove(777)
    rd.check(recommend(ix, reqs5, rd.K, ids=ids3), want5, "misfit removed")


# ------------------------------------------------------------------ errors
def test_invalid_arguments_are_refused_before_any_device_work(vdb):
    rows = bd.scaled(200, 8)
    ix = make_index(vdb, rd.EUCLID, rows)
    assert recommend(ix, [((1, 2), (3,))], 3)[2].tolist() == [3]
    stats = ix.recommend_stats()
    INV = vdb._ffi.ERR_INVALID_ARGUMENT
    ex = np.arange(70)
    cases = {
        "null ids": (None, [0, 2], [1]),
        "null offsets": (ex, None, [1]),
        "null n_pos": (ex, [0, 2], None),
        "offsets[0] != 0": (ex, [1, 3], [1]),
        "decreasing offsets": (ex, [0, 4, 2, 6], [1, 1, 1]),
        "no positive": (ex, [0, 2, 4], [1, 0]),
        "an empty request": (ex, [0, 2, 2], [1, 0]),
        "more positives than examples": (ex, [0, 2, 4], [1, 3]),
        "65 examples": (ex, [0, 2, 67], [1, 1]),
    }
    for what, (e, o, p) in cases.items():
        rc, oi, od, oc = raw_recommend(vdb, ix, e, o, p, None, 3, k=3, nq=1 if o is None else None)
        assert rc == INV, (what, rc, vdb._ffi.last_error())
        assert (oc == 12345).all() and (oi == POISON_ID).all(), what
    # offsets[nq] > 2^20: 16385 requests of 64 examples + one of 1
    nq = (1 << 20) // 64 + 1
    off = np.minimum(np.arange(nq + 1) * 64, (1 << 20) + 1)
    rc, _, _, oc = raw_recommend(vdb, ix, np.zeros((1 << 20) + 1, dtype=U64), off, np.ones(nq), None, 1, k=1)
    assert rc == INV and "2^20" in vdb._ffi.last_error()[0] and (oc == 12345).all()
    assert ix.recommend_stats() == stats                                       # no refused call reached the handle
    # 64 examples and a total of exactly 2^20 are legal sizes; kstride below k is the search's own refusal
    rc, _, _, oc = raw_recommend(vdb, ix, ex[:64], [0, 64], [40], None, 3, k=3)
    assert rc == 0 and oc.tolist() == [3]
    rc, _, _, _ = raw_recommend(vdb, ix, ex, [0, 2], [1], None, 2, k=3)
    assert rc == INV
    with pytest.raises(ValueError):
        ix.recommend_batch([[1]], [[2], [3]], 3)
    with pytest.raises(ValueError):
        ix.recommend_batch([[1]], [[]], 3, id_mask=np.zeros(4, dtype=U64), compiled_mask=object())


def test_not_found_names_the_first_absent_id(vdb):
    rows = bd.scaled(200, 8)
    ix = make_index(vdb, rd.EUCLID, rows)
    with pytest.raises(vdb.VectorNotFound) as e:
        ix.recommend_batch([[1, 2], [3, 900]], [[4, 777, 888], [999]], 3)      # array order: 1 2 4 777 888 3 900 999
    assert e.value.id == 777
    ix.remove(2)
    with pytest.raises(vdb.VectorNotFound) as e:
        ix.recommend_batch([[1, 2], [3, 900]], [[4, 777, 888], [999]], 3)
    assert e.value.id == 2
    rc, oi, _, oc = raw_recommend(vdb, ix, [1, 5, 2], [0, 1, 3], [1, 1], None, 3, k=3)
    assert rc == vdb._ffi.ERR_NOT_FOUND and "2" == vdb._ffi.last_error()[0].rsplit(": ", 1)[-1] and (oc == 12345).all()


def test_cosine_fold_of_p_and_minus_p_is_an_invalid_vector(vdb):
    n, d = 300, 16
    rows = bd.scaled(n, d).copy()
    rows[7] = -rows[3]
    rows[9] = rows[5]
    ix = make_index(vdb, rd.COSINE, rows)
    for pos, neg in (([3, 7], []), ([3], [3, 3, 7, 7]), ([5], [9, 9])):        # ap = 0 | ap + (ap - 0) with ap = p ... | p + (p - p) = p: fine
        q = rd.fold(rows, pos, neg)
        if not q.any():
            with pytest.raises(vdb.InvalidVector):
                ix.search_batch_arrays(q[None, :], 5)
            with pytest.raises(vdb.InvalidVector):
                ix.recommend_batch([pos, [1]], [neg, []], 5)
        else:
            rd.check(ix.recommend_batch([pos, [1]], [neg, []], 5), rd.expected(rd.COSINE, rows, [(pos, neg), ((1,), ())], 5), (pos, neg))
    assert not rd.fold(rows, [3, 7], []).any() and rd.fold(rows, [5], [9, 9]).any()
    eu = make_index(vdb, rd.EUCLID, rows)                                      # the same fold is an ordinary query under Euclid
    rd.check(eu.recommend_batch([[3, 7], [1]], [[], []], 5), rd.expected(rd.EUCLID, rows, [((3, 7), ()), ((1,), ())], 5), "euclid zero")


@pytest.mark.parametrize("metric", rd.METRICS)
def test_an_overflowing_fold_behaves_as_searching_with_that_vector(vdb, metric):
    n, d = 300, 16
    rows = bd.scaled(n, d).copy()
    rows[3] = F32(3e38)
    rows[7] = F32(3e38)
    ix = make_index(vdb, metric, rows)
    q = rd.fold(rows, [3, 7], [])
    assert np.isinf(q).all()                                                   # 3e38 + 3e38 overflows before the multiply by 0.5
    reqs = [((3, 7), ())] + [((10 + b, 30 + b), ()) for b in range(11)]     # twelve queries: neither call takes the direct path

    def outcome(f):
        try:
            return "ok", f()
        except vdb.VectorDbError as e:
            return type(e).__name__, None
    k = 5
    a, ares = outcome(lambda: ix.search_batch_arrays(rd.queries(rows, reqs), k + 2))
    b, bres = outcome(lambda: recommend(ix, reqs, k))
    print(f"metric {metric}: searching with the overflowed fold gives {a}, the recommend call {b}")
    assert a == b
    if a == "ok":
        for r, (p, _) in enumerate(reqs):
            si, sd = rd.strike(ares[0][r, :int(ares[2][r])], ares[1][r, :int(ares[2][r])], p, k)
            c = int(bres[2][r])
            assert c == len(si) and np.array_equal(bres[0][r, :c], si) and np.array_equal(bres[1][r, :c].view(np.uint32), sd.view(np.uint32))


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_recommend(vdb, device_filter):
    """VectorStore.recommend against the host composition it replaces: get, numpy fold, search_batch_prefiltered at k + m, strike
    by string id"""
    F = vdb.MetadataFilter
    n, d, k = 400, 12, 6
    rows = bd.scaled(n, d)
    st = vdb.VectorStore(vdb.DistanceMetric.DotProduct)
    if device_filter:
        st.set_device_filter(True)
    half = n // 2
    color = lambda i: ("blue", "green", "red")[i % 3]
    for i in range(half):                                                      # inserted rows: string ids, metadata objects
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata({"color": color(i)}))
    st.index().add_bulk(rows[half:], first_id=half)                             # bulk-attached rows: ids of their own
    st.attach_bulk_metadata(n - half, {"color": [color(i) for i in range(half, n)]}, ids=[f"bulk-{i}" for i in range(half, n)])
    assert st.device_filter() == device_filter
    name = lambda i: f"item-{i}" if i < half else f"bulk-{i}"
    reqs = [((2, half + 3, 7), (half, 1)), ((5,), ()), ((half + 1, 8), ()), ((11, 14, n - 1, 17), (20, 23, half + 5)), ((2, 2), (3,)),
            ((n - 2,), (n - 3,)), ((32, 35), ()), ((41,), ()), ((50, 53, 56), ()), ((62,), (65,)), ((71, half + 8), ()), ((80,), ())]

    def composed(p, ng, flt):
        vec = lambda i: np.asarray(st.get(name(i)).data, dtype=F32)
        stack = np.stack([vec(i) for i in p + ng])
        q = rd.fold(stack, range(len(p)), range(len(p), len(p) + len(ng)))
        m = len(p) + len(ng)
        if flt is None:
            (res,) = st.search_batch([(vdb.Vector(q), k + m)])
        else:
            (res,) = st.search_batch_prefiltered([(vdb.Vector(q), k + m)], flt)
        gone = {name(i) for i in p + ng}
        return [(r.id, r.distance) for r in res if r.id not in gone][:k]

    red = (np.arange(n) % 3) == 2
    for flt, live in ((None, None), (F.Eq("color", "red"), red.astype(np.uint8))):
        got = st.recommend_batch([([name(i) for i in p], [name(i) for i in ng]) for p, ng in reqs], k, flt)
        want = rd.expected(rd.DOT, rows, reqs, k, live=live)
        assert len(got) == len(reqs)
        for b, (p, ng) in enumerate(reqs):
            mine = [(r.id, r.distance) for r in got[b]]
            assert mine == composed(p, ng, flt), (b, flt is not None)
            assert [r.id for r in got[b]] == [name(int(i)) for i in want[b][0]], b
            assert np.array_equal(np.array([r.distance for r in got[b]], dtype=F32).view(np.uint32), want[b][1].view(np.uint32)), b
        one = st.recommend([name(i) for i in reqs[3][0]], [name(i) for i in reqs[3][1]], k, flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[3]]
    with pytest.raises(vdb.VectorNotFound):
        st.recommend([name(0), "nobody"], [], k)
    with pytest.raises(vdb.VectorNotFound):
        st.recommend([name(0)], ["bulk-3"], k)                                 # 3 is an inserted row: no bulk id names it
    # after an upsert of an example the fold reads the new vector
    st.insert_with_metadata(name(7), vdb.Vector((rows[7] * F32(-2.0)).astype(F32)), vdb.Metadata({"color": color(7)}))
    p, ng = reqs[0]
    got = st.recommend([name(i) for i in p], [name(i) for i in ng], k)
    assert [(r.id, r.distance) for r in got] == composed(p, ng, None)
    rows2 = rows.copy()
    rows2[7] = rows[7] * F32(-2.0)
    (oi, od), = rd.expected(rd.DOT, rows2, [reqs[0]], k)
    assert [r.id for r in got] == [name(int(i)) for i in oi]
    st.delete(name(5))
    with pytest.raises(vdb.VectorNotFound):
        st.recommend([name(5)], [], k)

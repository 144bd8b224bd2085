"""Diverse top-k: MMR re-ranking of the candidates on the device (vdb_flat_search_batch_mmr, csrc/kernels_mmr.hip, DESIGN.md
4.15).  Every case compares every query -- ids, pick order, distance bits, score bits and counts -- with the model of
tests/mmr_data.py: the contract of include/vdb_flat.h restated in numpy f32 over the CPU oracle's search and pair distances
(tests/test_mmr_cpu.py proves that the data makes a wrong pair order, a contracted score or a wrong tie-break visible)."""
import ctypes

import numpy as np
import pytest

import by_id_data as bd
import id_families as idf
import mmr_data as md
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


def noisy(rows, sel, scale=0.3, seed=1):
    rng = np.random.default_rng(20282 + seed)
    return np.ascontiguousarray((rows[np.asarray(sel)] + F32(scale) * rng.standard_normal((len(sel), rows.shape[1])).astype(F32)).astype(F32))


# ------------------------------------------------------------------ the cluster family
@pytest.mark.parametrize("metric", md.METRICS)
@pytest.mark.parametrize("dim", [17, 33])
def test_cluster_family_mixed_lambdas_and_ks(vdb, dim, metric):
    """8 queries (a batch the small-index search serves) and 9 with the direct path switched off (the tiered search); lambda mixes
    0, 0.5, 0.7 and 1, k mixes 1, 3 and 10"""
    rows, qs = md.cluster(dim, 9)
    ix = make_index(vdb, metric, rows)
    for nq, tiers in ((8, 0), (9, vdb.GpuFlatIndex.TIERS_NO_DIRECT)):
        ix.set_tiers(tiers)
        lams, ks = md.mixed(nq)
        want = md.expected(metric, rows, qs[:nq], ks, md.M, lams)
        got = ix.search_batch_mmr(qs[:nq], 0, md.M, lams, ks=ks)
        md.check(got, want, (dim, metric, nq))
        assert ix.mmr_stats()[:5] == md.stats(want, md.M), (ix.mmr_stats(), md.stats(want, md.M))
        assert ix.mmr_stats()[6:] == [0, 0]
        # a scalar lambda and a scalar k; the picks are not the plain top 10
        want = md.expected(metric, rows, qs[:nq], md.K, md.M, 0.7)
        got = ix.search_batch_mmr(qs[:nq], md.K, md.M, 0.7)
        md.check(got, want, (dim, metric, nq, "scalar"))
        plain = ix.search_batch_arrays(qs[:nq], md.K)
        assert any(got[0][b].tolist() != plain[0][b].tolist() for b in range(nq))


@pytest.mark.parametrize("metric", md.METRICS)
def test_lambda_one_is_the_plain_search(vdb, metric):
    rows, qs = md.cluster(33, 9)
    ix = make_index(vdb, metric, rows)
    gi, gd, gs, gc = ix.search_batch_mmr(qs, md.K, md.M, 1.0)
    pi, pd, pc = ix.search_batch_arrays(qs, md.K)
    assert same((gi, gd, gc), (pi, pd, pc))
    assert same((gs,), (pd,))                                                  # 1 * d - 0 * near = d


# ------------------------------------------------------------------ fold remainders
@pytest.mark.parametrize("metric", [md.EUCLID, md.COSINE])
@pytest.mark.parametrize("dim", [1, 15, 16, 31, 32, 48, 100])
def test_fold_remainders(vdb, dim, metric):
    """every remainder of the 16-element fold blocks; ld = dim rounded up to 32: the padded tail of a row must not enter a pair"""
    rows = bd.scaled(200, dim)
    qs = noisy(rows, [3, 50, 120, 199], seed=dim)
    ix = make_index(vdb, metric, rows)
    want = md.expected(metric, rows, qs, 5, 20, 0.6)
    md.check(ix.search_batch_mmr(qs, 5, 20, 0.6), want, (dim, metric))
    assert ix.mmr_stats()[:5] == md.stats(want, 20)


# ------------------------------------------------------------------ depth edges
def test_depth_edges(vdb):
    rows, qs = md.cluster(17, 9)
    ix = make_index(vdb, md.EUCLID, rows)
    want = md.expected(md.EUCLID, rows, qs[:3], 1, 1, 0.5)
    md.check(ix.search_batch_mmr(qs[:3], 1, 1, 0.5), want, "m = k = 1")
    assert ix.mmr_stats()[:5] == [3, 1, 3, 0, 3]
    want = md.expected_cached("m200", md.EUCLID, rows, qs[:2], 200, 200, 0.5)
    md.check(ix.search_batch_mmr(qs[:2], 200, 200, 0.5), want, "m = k = 200")
    assert ix.mmr_stats()[:5] == md.stats(want, 200)
    # a mask that leaves 5 rows eligible: c = 5, count = 5
    keep = [3, 50, 51, 300, 599]
    live = np.zeros(len(rows), dtype=np.uint8)
    live[keep] = 1
    mask, bits = id_mask(keep, len(rows))
    want = md.expected(md.EUCLID, rows, qs[:4], md.K, md.M, 0.5, live=live, stored=np.ones(len(rows), dtype=np.uint8))
    got = ix.search_batch_mmr(qs[:4], md.K, md.M, 0.5, id_mask=mask, mask_bits=bits)
    md.check(got, want, "5 eligible")
    assert got[3].tolist() == [5] * 4 and ix.mmr_stats()[:5] == [4, md.M, 20, 40, 20]
    # m above the index: the depth is the index
    small = make_index(vdb, md.EUCLID, rows[:7])
    want = md.expected(md.EUCLID, rows[:7], qs[:2], 7, 1024, 0.5)
    md.check(small.search_batch_mmr(qs[:2], 7, 1024, 0.5), want, "m above len")
    assert small.mmr_stats()[1] == 7


def test_the_deepest_candidate_list(vdb):
    """m = 1024 with k = 64 on 1300 x 16: every LDS entry in use, four candidates per thread"""
    rows = bd.scaled(1300, 16)
    qs = noisy(rows, [7, 1200], seed=5)
    ix = make_index(vdb, md.EUCLID, rows)
    want = md.expected_cached("m1024", md.EUCLID, rows, qs, 64, 1024, 0.5)
    md.check(ix.search_batch_mmr(qs, 64, 1024, 0.5), want, "m = 1024")
    assert ix.mmr_stats()[:5] == md.stats(want, 1024)


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize("metric", [md.EUCLID, md.DOT])
def test_triplicates(vdb, metric):
    rows, ids = bd.triplicates()
    qs = np.ascontiguousarray(rows[[3 * 5, 3 * 333 + 1, 3 * 699 + 2]] + F32(0.01))
    ix = make_index(vdb, metric, rows, ids=ids)
    want = md.expected(metric, rows, qs, 30, 30, 0.5, ids=ids)
    md.check(ix.search_batch_mmr(qs, 30, 30, 0.5), want, ("triplicates", metric))
    want = md.expected(metric, rows, qs, 12, 30, 0.3, ids=ids)
    md.check(ix.search_batch_mmr(qs, 12, 30, 0.3), want, ("triplicates, k 12", metric))


# ------------------------------------------------------------------ masks and mutations
@pytest.mark.parametrize("metric", [md.EUCLID, md.COSINE])
def test_masks_host_and_compiled(vdb, metric):
    rows, qs = md.cluster(33, 9)
    n = len(rows)
    ok = (np.arange(n) % 3) != 1
    mask, bits = id_mask(np.nonzero(ok)[0], n)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, ok.astype(np.int32))
    table.set_present(0, n, True)
    ix = make_index(vdb, metric, rows)
    want = md.expected(metric, rows, qs, md.K, md.M, 0.5, live=ok.astype(np.uint8), stored=np.ones(n, dtype=np.uint8))
    a = ix.search_batch_mmr(qs, md.K, md.M, 0.5, id_mask=mask, mask_bits=bits)
    md.check(a, want, "host mask")
    with table.compile([(vdb.MetaTable.EQ, 0, 1)], n) as cm:
        b = ix.search_batch_mmr(qs, md.K, md.M, 0.5, compiled_mask=cm)
    assert same(a, b)
    table.close()
    with pytest.raises(ValueError):
        ix.search_batch_mmr(qs, md.K, md.M, 0.5, id_mask=mask, compiled_mask=object())


def test_mutations(vdb):
    metric = md.EUCLID
    rows, qs = md.cluster(17, 9)
    n = len(rows)
    ids = np.arange(n, dtype=U64) * U64(3) + U64(1)
    ix = make_index(vdb, metric, rows, ids=ids)
    live = np.ones(n, dtype=np.uint8)
    md.check(ix.search_batch_mmr(qs, md.K, md.M, 0.5), md.expected(metric, rows, qs, md.K, md.M, 0.5, ids=ids), "fresh")
    # remove the nearest row of every query and every seventh row
    gone = set(int(i) for i in np.arange(0, n, 7))
    for oi, _ in md.oracle.search_batch(metric, rows, qs, 1, ids=ids):
        gone.add(int((int(oi[0]) - 1) // 3))
    for r in sorted(gone):
        ix.remove(int(ids[r]))
        live[r] = 0
    want = md.expected(metric, rows, qs, md.K, md.M, 0.5, ids=ids, live=live)
    before = ix.search_batch_mmr(qs, md.K, md.M, 0.5)
    md.check(before, want, "after remove")
    assert ix.compact() > 0                                                    # rows moved, ids did not: the id -> row map follows
    after = ix.search_batch_mmr(qs, md.K, md.M, 0.5)
    md.check(after, want, "after compact")
    assert same(before, after)
    # re-add removed ids with NEW vectors (staged, not flushed, when the call arrives)
    back = sorted(gone)[:20]
    new = np.ascontiguousarray((rows[back] * F32(1.01) + F32(0.02)).astype(F32))
    for r, v in zip(back, new):
        ix.add(int(ids[r]), vdb.Vector(v))
    rows2 = np.concatenate([rows, new])
    ids2 = np.concatenate([ids, ids[back]])
    live2 = np.concatenate([live, np.ones(len(back), dtype=np.uint8)])
    want = md.expected(metric, rows2, qs, md.K, md.M, 0.5, ids=ids2, live=live2)
    md.check(ix.search_batch_mmr(qs, md.K, md.M, 0.5), want, "re-added")
    assert any(np.isin(w["ids"], ids[back]).any() for w in want)


@pytest.mark.parametrize("family", idf.RELABELLED)
def test_wide_ids(vdb, family):
    rows, _ = md.cluster(17, 9)
    rows = rows[:300]
    ids = idf.family_ids(family, len(rows))
    qs = np.ascontiguousarray(rows[[299, 0, 150]] + F32(0.01))               # query 0 sits on the row with the largest id
    ix = make_index(vdb, md.DOT, rows, ids=ids)
    want = md.expected(md.DOT, rows, qs, md.K, md.M, 0.5, ids=ids)
    got = ix.search_batch_mmr(qs, md.K, md.M, 0.5)
    md.check(got, want, family)
    eu = make_index(vdb, md.EUCLID, rows, ids=ids)
    want = md.expected(md.EUCLID, rows, qs, md.K, md.M, 0.5, ids=ids)
    got = eu.search_batch_mmr(qs, md.K, md.M, 0.5)
    md.check(got, want, (family, "euclid"))
    if family == "top":
        assert int(got[0][0, 0]) == TOP                                        # 2^64 - 1 is a candidate and pick 1


# ------------------------------------------------------------------ the tiered pipeline on a larger index
@pytest.mark.parametrize("metric", [md.DOT, md.COSINE])
def test_scaled_family(vdb, metric):
    rows = bd.scaled()
    qs = noisy(rows, bd.spaced(bd.N, 16), scale=0.1, seed=9)
    ix = make_index(vdb, metric, rows)
    want = md.expected_cached(("scaled", metric), metric, rows, qs, 10, 64, 0.5)
    md.check(ix.search_batch_mmr(qs, 10, 64, 0.5), want, ("scaled", metric))
    assert ix.mmr_stats()[:5] == md.stats(want, 64)


# ------------------------------------------------------------------ errors
def raw_mmr(vdb, ix, qs, k, m, lam, ks=None, lams=None, kstride=None, null=(), nq=None, dim=None):
    """the C entry point itself, with poisoned outputs; `null` names the arrays passed as null pointers"""
    L = vdb._ffi.lib()
    u64p, szp, fp = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_size_t, ctypes.c_float))
    qs = np.ascontiguousarray(qs, dtype=F32)
    nq = qs.shape[0] if nq is None else nq
    dim = qs.shape[1] if dim is None else dim
    kmax = int(k) if ks is None else int(max(ks))
    kstride = max(kmax, 1) if kstride is None else kstride
    oi = np.full((nq, max(kstride, 1)), POISON_ID, dtype=U64)
    od = np.full((nq, max(kstride, 1)), POISON_D, dtype=np.uint32).view(F32)
    os_ = np.full((nq, max(kstride, 1)), POISON_D, dtype=np.uint32).view(F32)
    oc = np.full(nq, 12345, dtype=np.uintp)
    ks_a = None if ks is None else np.ascontiguousarray(ks, dtype=np.uintp)
    lams_a = None if lams is None else np.ascontiguousarray(lams, dtype=F32)
    ptr = lambda name, a, t: None if (a is None or name in null) else a.ctypes.data_as(t)
    rc = L.vdb_flat_search_batch_mmr(ix._h, ptr("queries", qs, fp), nq, dim, ptr("ks", ks_a, szp), int(k), int(m), ptr("lambdas", lams_a, fp),
                                     float(lam), None, 0, kstride, ptr("ids", oi, u64p), ptr("dists", od, fp), ptr("scores", os_, fp),
                                     ptr("counts", oc, szp))
    return rc, oi, od, os_, oc


def test_invalid_arguments_are_refused_before_any_device_work(vdb):
    rows, qs = md.cluster(17, 9)
    ix = make_index(vdb, md.EUCLID, rows)
    q = qs[:2]
    assert ix.search_batch_mmr(q, 3, 8, 0.5)[3].tolist() == [3, 3]
    stats = ix.mmr_stats()
    INV = vdb._ffi.ERR_INVALID_ARGUMENT
    cases = {
        "null queries": dict(k=3, m=8, lam=0.5, null=("queries",)),
        "null ids": dict(k=3, m=8, lam=0.5, null=("ids",)),
        "null dists": dict(k=3, m=8, lam=0.5, null=("dists",)),
        "null counts": dict(k=3, m=8, lam=0.5, null=("counts",)),
        "NaN lambda": dict(k=3, m=8, lam=float("nan")),
        "lambda below 0": dict(k=3, m=8, lam=-0.001),
        "lambda above 1": dict(k=3, m=8, lam=1.001),
        "one bad lambda in the array": dict(k=3, m=8, lam=0.5, lams=[0.5, 1.5]),
        "a NaN lambda in the array": dict(k=3, m=8, lam=0.5, lams=[float("nan"), 0.5]),
        "m = 0": dict(k=3, m=0, lam=0.5),
        "m = 1025": dict(k=3, m=1025, lam=0.5),
        "k above m": dict(k=9, m=8, lam=0.5),
        "max ks above m": dict(k=0, m=8, lam=0.5, ks=[2, 9]),
        "kstride below k": dict(k=3, m=8, lam=0.5, kstride=2),
    }
    for what, kw in cases.items():
        rc, oi, od, os_, oc = raw_mmr(vdb, ix, q, **kw)
        assert rc == INV, (what, rc, vdb._ffi.last_error())
        assert (oc == 12345).all() and (oi == POISON_ID).all(), what
    assert ix.mmr_stats() == stats                                             # no refused call reached the handle
    # the limits themselves are legal, and the scores are optional
    rc, oi, od, os_, oc = raw_mmr(vdb, ix, q, 3, 1024, 1.0, null=("scores",))
    assert rc == 0 and oc.tolist() == [3, 3] and (os_.view(np.uint32) == POISON_D).all()
    rc, _, _, _, oc = raw_mmr(vdb, ix, q, 8, 8, 0.0)
    assert rc == 0 and oc.tolist() == [8, 8]
    # k = 0 answers before any other check
    rc, oi, _, _, oc = raw_mmr(vdb, ix, q, 0, 0, 7.0)
    assert rc == 0 and oc.tolist() == [0, 0] and (oi == POISON_ID).all()
    rc, _, _, _, oc = raw_mmr(vdb, ix, q, 0, 8, 0.5, ks=[0, 0])
    assert rc == 0 and oc.tolist() == [0, 0]
    # per-query ks with a zero among them
    rc, oi, od, os_, oc = raw_mmr(vdb, ix, q, 0, 8, 0.5, ks=[0, 4])
    assert rc == 0 and oc.tolist() == [0, 4] and (oi[0] == POISON_ID).all()
    md.check((oi, od, os_, oc), md.expected(md.EUCLID, rows, q, [0, 4], 8, 0.5), "ks 0, 4")
    assert (oi[1, 4:] == POISON_ID).all()


def test_sharded_handle_is_refused(vdb):
    rows, qs = md.cluster(17, 9)
    sh = make_index(vdb, md.EUCLID, rows, devices=[0, 0])
    rc, _, _, _, oc = raw_mmr(vdb, sh, qs[:2], 3, 8, 0.5)
    assert rc == vdb._ffi.ERR_INVALID_ARGUMENT and "sharded" in vdb._ffi.last_error()[0] and (oc == 12345).all()
    out = (ctypes.c_uint64 * 8)()
    assert vdb._ffi.lib().vdb_flat_mmr_stats(sh._h, out) == vdb._ffi.ERR_INVALID_ARGUMENT


def test_empty_index_and_empty_batch(vdb):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False)
    q = np.ones((2, 4), dtype=F32)
    rc, oi, _, _, oc = raw_mmr(vdb, ix, q, 3, 8, 0.5)
    assert rc == 0 and oc.tolist() == [0, 0] and (oi == POISON_ID).all()
    rc, _, _, _, oc = raw_mmr(vdb, ix, q, 9, 0, 2.0)                           # an empty index answers before any other check
    assert rc == 0 and oc.tolist() == [0, 0]
    gi, gd, gs, gc = ix.search_batch_mmr(np.zeros((0, 4), dtype=F32), 3, 8, 0.5)
    assert gc.size == 0 and ix.mmr_stats()[0] == 0


def test_a_nan_pair_is_an_error_and_a_nan_score_ranks_last(vdb):
    """rows 1 and 2 hold +inf: both score inf - inf = NaN after the finite pick, the lower position wins (k = 2); a third pick
    evaluates D(row 1, row 2) = NaN, which is VDB_ERR_NAN (k = 3).  Error returns, not faults."""
    rows, q = md.inf_case()
    ix = make_index(vdb, md.EUCLID, rows)
    (w,) = md.expected(md.EUCLID, rows, q, 2, 3, 0.5)
    assert w["ids"].tolist() == [0, 1] and np.isnan(w["scores"][1])
    got = ix.search_batch_mmr(q, 2, 3, 0.5)
    md.check(got, [w], "k = 2")
    assert ix.mmr_stats()[:5] == [1, 3, 3, 2, 2]
    rc, _, _, _, _ = raw_mmr(vdb, ix, q, 3, 3, 0.5)
    assert rc == vdb._ffi.ERR_NAN, (rc, vdb._ffi.last_error())
    with pytest.raises(vdb.VectorDbError):
        ix.search_batch_mmr(q, 3, 3, 0.5)
    # lambda = 1 does not save it: the pair is still evaluated
    rc, _, _, _, _ = raw_mmr(vdb, ix, q, 3, 3, 1.0)
    assert rc == vdb._ffi.ERR_NAN
    md.check(ix.search_batch_mmr(q, 2, 3, 0.5), [w], "after the error")


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_search_mmr(vdb, device_filter):
    F = vdb.MetadataFilter
    rows, qs = md.cluster(17, 9)
    n, k = 240, 6
    rows = rows[:n]
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    if device_filter:
        st.set_device_filter(True)
    color = lambda i: ("blue", "green", "red")[i % 3]
    for i in range(n):
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata({"color": color(i)}))
    assert st.device_filter() == device_filter
    red = (np.arange(n) % 3) == 2
    for flt, live in ((None, None), (F.Eq("color", "red"), red.astype(np.uint8))):
        stored = None if live is None else np.ones(n, dtype=np.uint8)
        want = md.expected(md.EUCLID, rows, qs[:4], k, 32, 0.5, live=live, stored=stored)      # the default depth: min(max(4 k, 32), 1024)
        got = st.search_mmr_batch([vdb.Vector(q) for q in qs[:4]], k, flt=flt)
        assert len(got) == 4
        for b, w in enumerate(want):
            assert [r.id for r in got[b]] == [f"item-{int(i)}" for i in w["ids"]], (b, flt is not None)
            assert np.array_equal(np.array([r.distance for r in got[b]], dtype=F32).view(np.uint32), w["dists"].view(np.uint32)), b
        one = st.search_mmr(vdb.Vector(qs[2]), k, flt=flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[2]]
        want = md.expected(md.EUCLID, rows, qs[:2], k, 50, 0.8, live=live, stored=stored)
        got = st.search_mmr_batch([vdb.Vector(q) for q in qs[:2]], k, lam=0.8, candidates=50, flt=flt)
        for b, w in enumerate(want):
            assert [r.id for r in got[b]] == [f"item-{int(i)}" for i in w["ids"]], (b, "lam 0.8")
    assert vdb.VectorStore(vdb.DistanceMetric.Euclidean).search_mmr(vdb.Vector(qs[0]), k) == []

"""Recommend by best score (vdb_flat_recommend_best_batch, csrc/kernels_recommend_best.hip): nearest to ANY
positive, vetoed by the negatives.  Every case compares every request -- ids, order, dp bits, dn bits, counts -- with the
definition computed from the CPU oracle's full rankings, and vdb_flat_recommend_best_stats with the restatement of the list route
(tests/recommend_best_data.py; tests/test_recommend_best_cpu.py proves that the restatement equals the definition and that the
veto families end at list stage 0, list stage 1 and the exact scan).  Every family runs on more than one route and the bits must
be the same.  No tolerance anywhere."""
import numpy as np
import pytest

import by_id_data as bd
import id_families as idf
import recommend_data as rd
import recommend_best_data as rb
from conftest import load_package
from split_schedule import SPLIT, Rule

pytestmark = pytest.mark.gpu

U64, F32 = np.uint64, np.float32
ROUTES = (rb.AUTO, rb.LISTS, rb.SCAN)


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    yield v
    _INDEX.clear()


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


def run(ix, reqs, k, ids=None, route=rb.AUTO, **kw):
    ix.debug_set_recommend_best_route(route)
    try:
        pos, neg = rb.split(reqs, ids)
        return ix.recommend_best_batch(pos, neg, k, **kw)
    finally:
        ix.debug_set_recommend_best_route(rb.AUTO)


def trim(got):
    """the valid part of every list: what two routes must agree on bit for bit"""
    gi, gd, gn, gc = got
    return [(gi[b, :int(c)].copy(), gd[b, :int(c)].copy(), gn[b, :int(c)].copy()) for b, c in enumerate(gc)]


def check_routes(ix, key, metric, rows, reqs, k, ids=None, live=None, mask=None, routes=ROUTES, **kw):
    """every route against the definition and the predicted stats; the same bits on all of them"""
    seen = []
    for route in routes:
        got = run(ix, reqs, k, ids=ids, route=route, **kw)
        st = ix.recommend_best_stats()
        want, stages, pst = rb.expected(key, metric, rows, reqs, k, ids=ids, live=live, mask=mask, route=route)
        rb.check(got, want, (key, metric, route))
        assert st == list(pst), (key, metric, route, st, pst, stages)
        seen.append(trim(got))
    for other in seen[1:]:
        for x, y in zip(seen[0], other):
            assert same(x, y), (key, metric)
    return seen[0]


_INDEX = {}


def scaled_index(vdb, metric):
    if metric not in _INDEX:
        _INDEX[metric] = make_index(vdb, metric, bd.scaled())
    return _INDEX[metric]


# ------------------------------------------------------------------ the families, 600 to 4000 rows
@pytest.mark.parametrize("metric", rb.METRICS)
@pytest.mark.parametrize("name", sorted(rb.FAMILIES))
def test_families_on_every_route(vdb, name, metric):
    rows, ids, reqs = rb.FAMILIES[name]()
    ix = make_index(vdb, metric, rows, ids=ids)
    check_routes(ix, name, metric, rows, reqs, rb.K, ids=ids)
    if metric != rb.DOT and name in ("trap", "veto100", "veto1500"):
        stage = {"trap": 0, "veto100": 1, "veto1500": rb.STAGE_SCAN}[name]
        run(ix, reqs, rb.K, ids=ids)
        st = ix.recommend_best_stats()
        assert st[2 + stage] == 1 and sum(st[2:5]) == 1, (name, st)          # automatic: stage 0, stage 1, the scan


def test_inf_rows_and_the_nan_positive_on_both_routes(vdb):
    rows, ids, reqs = rb.inf_family()
    ix = make_index(vdb, rb.EUCLID, rows)
    got = check_routes(ix, "inf", rb.EUCLID, rows, reqs, 1000)
    assert np.isinf(got[1][1][-len(rb.INF_ROWS):]).all() and len(got[1][0]) == rb.INF_N - 1
    for route in (rb.LISTS, rb.SCAN):
        with pytest.raises(vdb.NanDistance):
            run(ix, rb.inf_nan_request(), rb.K, route=route)
        with pytest.raises(vdb.NanDistance):                                   # ... also when the NaN request is not the only one
            run(ix, reqs + rb.inf_nan_request(), rb.K, route=route)


# ------------------------------------------------------------------ index sizes that reach each tier
@pytest.mark.parametrize("metric", rb.METRICS)
def test_20000_rows_above_the_dense_tier(vdb, metric):
    rows = bd.scaled()
    reqs = rd.scaled_requests()[:10]
    ix = scaled_index(vdb, metric)
    check_routes(ix, "scaled10", metric, rows, reqs, rb.K)


def test_66000_x_32_above_the_screening_floor(vdb):
    n, metric = 66000, rb.COSINE
    rows = bd.scaled(n, 32)
    reqs = (((3, 77, 1000), (20,)), ((65000,), ()), ((5, 6, 7, 8, 9, 40000, 40001), (100, 200, 300)))
    ix = make_index(vdb, metric, rows)
    check_routes(ix, "big66x32", metric, rows, reqs, rb.K)
    run(ix, reqs, rb.K, route=rb.LISTS)
    assert ix.last_stats()["bf16_screen"] == 1, ix.last_stats()               # the list search was the bf16 screening tier


def test_66000_rows_screened_and_from_split_rows(vdb):
    """above BF16_MIN_ROWS the list search is the bf16 screening tier; from a SPLIT store the gather reads f32 rows (back), the
    search converts again (mode 2), the veto reads f32 rows (back): the rule split_schedule applies to by-id and MMR reads"""
    n, d, metric = 66000, 64, rb.EUCLID
    rows = bd.scaled(n, d)
    reqs = (((3, 77, 1000), (20,)), ((65000,), ()), ((5, 6, 7, 8, 9, 40000, 40001), (100, 200, 300)))
    ix = make_index(vdb, metric, rows)
    ix.set_split(2)
    rule = Rule(2, n)
    want, stages, pst = rb.expected("big66", metric, rows, reqs, rb.K)
    assert set(stages) == {0}
    for _ in range(2):
        ix.search_batch_arrays(rows[:2], 5)
        rule.search(nq=2)
        assert ix.layout()[0] == SPLIT and tuple(ix.layout()) == rule.expect()
        got = run(ix, reqs, rb.K)
        rule.search(nq=sum(len(p) for p, _ in reqs), by_id=True)
        rule.reader()
        rb.check(got, want, "66000 from SPLIT")
        assert ix.recommend_best_stats() == list(pst)
        assert ix.last_stats()["bf16_screen"] == 1, ix.last_stats()
        assert tuple(ix.layout()) == rule.expect(), (ix.layout(), rule.expect())
    scan = run(ix, reqs, rb.K, route=rb.SCAN)
    rule.reader()
    rb.check(scan, want, "66000 scan")
    assert same(trim(scan), trim(got)) and tuple(ix.layout()) == rule.expect()


# ------------------------------------------------------------------ masks, removed rows, compaction, the id space
def test_masks_removed_rows_and_compaction(vdb):
    rows, _, reqs = rb.fold_family(33)
    n = len(rows)
    rng = np.random.default_rng(7)
    mask_on = (rng.random(n) < 0.5).astype(np.uint8)
    flat = np.array([e for p, g in reqs for e in p + g])
    assert mask_on[flat].any() and not mask_on[flat].all()                     # some examples are masked out: still examples
    mask, bits = id_mask(np.nonzero(mask_on)[0], n)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, mask_on.astype(np.int32))
    table.set_present(0, n, True)
    for metric in rb.METRICS:
        ix = make_index(vdb, metric, rows)
        a = check_routes(ix, "fold33-mask", metric, rows, reqs, rb.K, mask=mask_on, id_mask=mask, mask_bits=bits)
        with table.compile([(vdb.MetaTable.EQ, 0, 1)], n) as cm:
            for route in (rb.LISTS, rb.SCAN):
                assert same(trim(run(ix, reqs, rb.K, route=route, compiled_mask=cm)), a), (metric, route)
        # removed rows (no example among them), with and without the mask; then the same after compact()
        live = np.ones(n, dtype=np.uint8)
        for r in rng.choice(n, 80, replace=False):
            if r not in flat:
                ix.remove(int(r))
                live[r] = 0
        b = check_routes(ix, "fold33-dead%d" % metric, metric, rows, reqs, rb.K, live=live)
        c = check_routes(ix, "fold33-deadmask%d" % metric, metric, rows, reqs, rb.K, live=live, mask=mask_on, id_mask=mask, mask_bits=bits)
        assert ix.compact() > 0
        for route in ROUTES:
            assert same(trim(run(ix, reqs, rb.K, route=route)), b), (metric, route)
            assert same(trim(run(ix, reqs, rb.K, route=route, id_mask=mask, mask_bits=bits)), c), (metric, route)
    table.close()


@pytest.mark.parametrize("family", ["across63", "top"])
def test_ids_that_are_not_monotone_and_reach_2_to_the_64(vdb, family):
    rows, _, reqs = rb.fold_family(33)
    n = len(rows)
    ids = idf.family_ids(family, n, idf.permutation(n))
    assert (ids[1:] < ids[:-1]).any() and int(ids.max()) >= 2 ** 63
    if family == "top":
        assert int(ids.max()) == 2 ** 64 - 1                                   # no id value is a flag
    for metric in (rb.EUCLID, rb.DOT):
        ix = make_index(vdb, metric, rows, ids=ids)
        check_routes(ix, "fold33-" + family, metric, rows, reqs, rb.K, ids=ids)


# ------------------------------------------------------------------ counts
def test_per_request_k_k_above_len_short_lists_and_an_empty_batch(vdb):
    rows, _, reqs = rb.fold_family(64)
    n = len(rows)
    ks = np.array([1 + (37 * b) % 90 for b in range(len(reqs))])
    ks[3] = 0
    for metric in (rb.EUCLID, rb.COSINE):
        ix = make_index(vdb, metric, rows)
        got = check_routes(ix, "fold64-ks", metric, rows, reqs, ks)
        for (gi, _, _), kb in zip(got, ks):
            assert len(gi) <= kb
        # k above len: every kept row of every request, in order -- short lists, not an error
        full = check_routes(ix, "fold64-all", metric, rows, reqs, 5000)
        counts = [len(gi) for gi, _, _ in full]
        assert max(counts) <= n - 1 and min(counts) < n - 64, counts           # (the vetoes leave some requests a short list)
        assert full[0][0].size == n - 1 and np.isinf(full[0][2]).all()         # one positive, no negative: everybody else
    ix = make_index(vdb, rb.EUCLID, rows)
    gi, gd, gn, gc = ix.recommend_best_batch([], [], 5)
    assert gc.size == 0 and ix.recommend_best_stats() == [0] * 8
    gi, gd, gn, gc = ix.recommend_best_batch([[1, 2]], [[3]], 0)
    assert gc.tolist() == [0]
    with pytest.raises(vdb.VectorDbError):                                     # more rows per request than the call returns
        make_index(vdb, rb.EUCLID, bd.scaled(1500, 8)).recommend_best_batch([[1]], [[]], 1025)


@pytest.mark.parametrize("metric", rb.METRICS)
def test_one_positive_and_no_negative_is_search_by_id(vdb, metric):
    sel = bd.spaced(bd.N, 24)
    ix = scaled_index(vdb, metric)
    reqs = [((int(r),), ()) for r in sel]
    want = ix.search_batch_by_id(sel.astype(U64), bd.K)
    ok = (np.arange(bd.N) % 2) == 0
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    want_m = ix.search_batch_by_id(sel.astype(U64), bd.K, id_mask=mask, mask_bits=bits)
    for route in ROUTES:
        gi, gd, gn, gc = run(ix, reqs, bd.K, route=route)
        assert same((gi, gd, gc), want), (metric, route)
        assert np.isinf(gn).all()
        gi, gd, gn, gc = run(ix, reqs, bd.K, route=route, id_mask=mask, mask_bits=bits)
        assert same((gi, gd, gc), want_m), (metric, route, "masked")


# ------------------------------------------------------------------ errors
def test_errors(vdb):
    n, d = 300, 16
    rows = bd.scaled(n, d).copy()
    ix = make_index(vdb, rb.EUCLID, rows)
    for route in (rb.LISTS, rb.SCAN):
        ix.debug_set_recommend_best_route(route)
        with pytest.raises(vdb.VectorNotFound) as e:
            ix.recommend_best_batch([[1, 2], [3, 900]], [[4, 777], [999]], 3)  # array order: 1 2 4 777 ...
        assert e.value.id == 777
    ix.debug_set_recommend_best_route(rb.AUTO)
    ix.remove(2)
    with pytest.raises(vdb.VectorNotFound) as e:
        ix.recommend_best_batch([[1, 2]], [[4]], 3)
    assert e.value.id == 2
    odd = np.ones(d + 3, dtype=F32)
    ix.add(7777, vdb.Vector(odd))
    with pytest.raises(vdb.DimensionMismatch) as e1:
        ix.recommend_batch([[7777, 1]], [[]], 3)
    with pytest.raises(vdb.DimensionMismatch) as e2:
        ix.recommend_best_batch([[7777, 1]], [[]], 3)
    assert (e2.value.expected, e2.value.actual) == (e1.value.expected, e1.value.actual)
    with pytest.raises(vdb.DimensionMismatch):
        ix.recommend_best_batch([[1]], [[5]], 3)
    ix.remove(7777)
    assert ix.recommend_best_batch([[1]], [[5]], 3)[3].tolist() == [3]
    # Cosine: a zero-norm example, and any live zero-norm row, is an invalid vector on every route
    zrows = rows.copy()
    zrows[9] = 0
    cz = make_index(vdb, rb.COSINE, zrows)
    for route in ROUTES:
        for pos, neg in (([9], []), ([1], [9]), ([1], [2])):
            with pytest.raises(vdb.InvalidVector):
                run(cz, [(pos, neg)], 3, route=route)
    cz.remove(9)
    want = rb.definition("zero-removed", rb.COSINE, zrows, [((1,), (2,))], 3, live=(np.arange(n) != 9).astype(np.uint8))
    for route in ROUTES:
        rb.check(run(cz, [((1,), (2,))], 3, route=route), want, route)
    with pytest.raises(ValueError):
        ix.recommend_best_batch([[1]], [[2], [3]], 3)


def test_a_sharded_handle_is_refused(vdb):
    sh = make_index(vdb, rb.EUCLID, bd.scaled(3000, 16), devices=[0, 0])
    with pytest.raises(vdb.VectorDbError) as e:
        sh.recommend_best_batch([[1, 2]], [[3]], 3)
    assert "sharded" in str(e.value)
    assert sh.recommend_batch([[1, 2]], [[3]], 3)[2].tolist() == [3]           # (the average-vector recommend serves it)


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_recommend_best(vdb, device_filter):
    F = vdb.MetadataFilter
    n, d, k = 400, 12, 6
    rows = bd.scaled(n, d)
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    if device_filter:
        st.set_device_filter(True)
    half = n // 2
    color = lambda i: ("blue", "green", "red")[i % 3]
    for i in range(half):
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata({"color": color(i)}))
    st.index().add_bulk(rows[half:], first_id=half)
    st.attach_bulk_metadata(n - half, {"color": [color(i) for i in range(half, n)]}, ids=[f"bulk-{i}" for i in range(half, n)])
    assert st.device_filter() == device_filter
    name = lambda i: f"item-{i}" if i < half else f"bulk-{i}"
    reqs = [((2, half + 3, 7), (half, 1)), ((5,), ()), ((half + 1, 8), ()), ((11, 14, n - 1, 17), (20, 23, half + 5)), ((2, 2), (3,)),
            ((n - 2,), (n - 3,))]
    red = (np.arange(n) % 3) == 2
    for flt, mask in ((None, None), (F.Eq("color", "red"), red.astype(np.uint8))):
        got = st.recommend_best_batch([([name(i) for i in p], [name(i) for i in g]) for p, g in reqs], k, flt)
        want = rb.definition(("store", flt is not None), rb.EUCLID, rows, reqs, k, mask=mask)
        assert len(got) == len(reqs)
        for b in range(len(reqs)):
            assert [r.id for r in got[b]] == [name(int(i)) for i in want[b][0]], b
            assert np.array_equal(np.array([r.distance for r in got[b]], dtype=F32).view(np.uint32), want[b][1].view(np.uint32)), b
        one = st.recommend_best([name(i) for i in reqs[3][0]], [name(i) for i in reqs[3][1]], k, flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[3]]
    with pytest.raises(vdb.VectorNotFound):
        st.recommend_best([name(0), "nobody"], [], k)

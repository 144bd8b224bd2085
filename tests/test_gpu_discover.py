"""Discovery search (vdb_flat_discover_batch, csrc/kernels_discover.hip): a target ranked inside context pairs.
Every case compares every request -- ids, order, distance bits, ranks, counts -- with the definition computed from the CPU oracle's
full rankings, and vdb_flat_discover_stats with the restatement of the list route (tests/discover_data.py;
tests/test_discover_cpu.py proves that the restatement equals the definition and that the families end at list stage 0, list stage
1 and the exact scan).  Every family runs on all three routes and the bits must be the same.  No tolerance anywhere."""
import numpy as np
import pytest

import by_id_data as bd
import id_families as idf
import discover_data as dd
from conftest import load_package
from split_schedule import SPLIT

pytestmark = pytest.mark.gpu

U64, F32, U32 = np.uint64, np.float32, np.uint32
ROUTES = (dd.AUTO, dd.LISTS, dd.SCAN)


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


def run(ix, reqs, k, ids=None, route=dd.AUTO, **kw):
    ix.debug_set_discover_route(route)
    try:
        targets, pairs = dd.split(reqs, ids)
        return ix.discover_batch(targets, pairs, k, **kw)
    finally:
        ix.debug_set_discover_route(dd.AUTO)


def trim(got):
    """the valid part of every list: what two routes must agree on bit for bit"""
    gi, gd, gr, gc = got
    return [(gi[b, :int(c)].copy(), gd[b, :int(c)].copy(), gr[b, :int(c)].copy()) for b, c in enumerate(gc)]


def check_routes(ix, key, metric, rows, reqs, k, ids=None, live=None, mask=None, routes=ROUTES, **kw):
    """every route against the definition and the predicted stats; the same bits on all of them"""
    seen = []
    for route in routes:
        got = run(ix, reqs, k, ids=ids, route=route, **kw)
        st = ix.discover_stats()
        want, stages, pst = dd.expected(key, metric, rows, reqs, k, ids=ids, live=live, mask=mask, route=route)
        dd.check(got, want, (key, metric, route))
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
@pytest.mark.parametrize("metric", dd.METRICS)
@pytest.mark.parametrize("name", sorted(dd.FAMILIES))
def test_families_on_every_route(vdb, name, metric):
    rows, ids, reqs, k = dd.FAMILIES[name]()
    ix = make_index(vdb, metric, rows, ids=ids)
    check_routes(ix, "d-" + name, metric, rows, reqs, k, ids=ids)
    if metric != dd.DOT and name in dd.STAGES:
        _, stages, _ = dd.expected("d-" + name, metric, rows, reqs, k, ids=ids)
        for b, stage in dd.STAGES[name].items():
            assert stages[b] == stage, (name, metric, stages)                  # (the stats matched: the engine went the same way)


def test_inf_rows_a_nan_context_distance_and_the_nan_target_on_every_route(vdb):
    rows, ids, reqs, k = dd.inf_family()
    ix = make_index(vdb, dd.EUCLID, rows)
    got = check_routes(ix, "d-inf", dd.EUCLID, rows, reqs, k)
    assert np.isinf(got[0][1][-len(dd.INF_ROWS):]).all() and len(got[0][0]) == dd.INF_N - 3
    for route in ROUTES:
        with pytest.raises(vdb.NanDistance):
            run(ix, dd.inf_nan_request(), dd.K, route=route)
        with pytest.raises(vdb.NanDistance):                                   # ... also when the NaN request is not the only one
            run(ix, reqs + dd.inf_nan_request(), dd.K, route=route)
    # the NaN target distance stands at an EXAMPLE only (the other +inf rows are removed): still an error -- they are struck afterwards
    ix.remove(dd.INF_ROWS[1])
    ix.remove(dd.INF_ROWS[2])
    for route in ROUTES:
        with pytest.raises(vdb.NanDistance):
            run(ix, dd.inf_nan_request(), dd.K, route=route)


# ------------------------------------------------------------------ index sizes that reach the other search tiers
@pytest.mark.parametrize("metric", dd.METRICS)
def test_20000_rows_above_the_dense_tier(vdb, metric):
    rows = bd.scaled()
    reqs = ((5, ((100, 200), (300, 400))), (19999, ()), (7, ((7, 8), (9, 10), (11, 12), (13, 14), (15, 16))))
    check_routes(scaled_index(vdb, metric), "d-scaled", metric, rows, reqs, dd.K)


def test_66000_x_64_a_split_handle_and_a_plain_one_give_the_same_bits(vdb):
    """above the screening floor a set_split(2) handle converts its rows to the SPLIT layout at a screened search; the gather, the
    rank kernel and the scan ask for f32 rows, which converts them back: the same bits from both handles on every route"""
    n, d, metric = 66000, 64, dd.EUCLID
    rows = bd.scaled(n, d)
    reqs = ((3, ((77, 1000), (20, 21))), (65000, ()), (5, ((6, 7), (8, 9), (40000, 40001))))
    plain = make_index(vdb, metric, rows)
    base = check_routes(plain, "d-big66", metric, rows, reqs, dd.K)
    ix = make_index(vdb, metric, rows)
    ix.set_split(2)
    for route in ROUTES:
        ix.search_batch_arrays(rows[:2], 5)
        assert ix.layout()[0] == SPLIT
        got = run(ix, reqs, dd.K, route=route)
        for x, y in zip(trim(got), base):
            assert same(x, y), route
        assert ix.discover_stats() == list(dd.expected("d-big66", metric, rows, reqs, dd.K, route=route)[2])


# ------------------------------------------------------------------ masks, removed rows, compaction, the id space
def test_masks_removed_rows_and_compaction(vdb):
    rows, _, reqs, k = dd.ragged()
    n = len(rows)
    rng = np.random.default_rng(7)
    mask_on = (rng.random(n) < 0.5).astype(np.uint8)
    flat = np.array(sorted(set(e for r in reqs for e in dd.examples(r))))
    assert mask_on[flat].any() and not mask_on[flat].all()                     # some examples are masked out: still examples
    mask, bits = id_mask(np.nonzero(mask_on)[0], n)
    table = vdb.MetaTable(0)
    table.set_codes(0, 0, mask_on.astype(np.int32))
    table.set_present(0, n, True)
    for metric in dd.METRICS:
        ix = make_index(vdb, metric, rows)
        a = check_routes(ix, "d-ragged-mask", metric, rows, reqs, k, mask=mask_on, id_mask=mask, mask_bits=bits)
        with table.compile([(vdb.MetaTable.EQ, 0, 1)], n) as cm:
            for route in ROUTES:
                for x, y in zip(trim(run(ix, reqs, k, route=route, compiled_mask=cm)), a):
                    assert same(x, y), (metric, route)
        # removed rows (no example among them), with and without the mask; then the same after compact()
        live = np.ones(n, dtype=np.uint8)
        for r in rng.choice(n, 80, replace=False):
            if r not in flat:
                ix.remove(int(r))
                live[r] = 0
        b = check_routes(ix, "d-ragged-dead%d" % metric, metric, rows, reqs, k, live=live)
        c = check_routes(ix, "d-ragged-deadmask%d" % metric, metric, rows, reqs, k, live=live, mask=mask_on, id_mask=mask, mask_bits=bits)
        assert ix.compact() > 0
        for route in ROUTES:
            for x, y in zip(trim(run(ix, reqs, k, route=route)), b):
                assert same(x, y), (metric, route)
            for x, y in zip(trim(run(ix, reqs, k, route=route, id_mask=mask, mask_bits=bits)), c):
                assert same(x, y), (metric, route)
    table.close()


@pytest.mark.parametrize("family", ["across63", "top"])
def test_ids_that_are_not_monotone_and_reach_2_to_the_64(vdb, family):
    rows, _, reqs, k = dd.ragged()
    n = len(rows)
    ids = idf.family_ids(family, n, idf.permutation(n))
    assert (ids[1:] < ids[:-1]).any() and int(ids.max()) >= 2 ** 63
    if family == "top":
        assert int(ids.max()) == 2 ** 64 - 1                                   # no id value is a flag
    for metric in (dd.EUCLID, dd.DOT):
        ix = make_index(vdb, metric, rows, ids=ids)
        check_routes(ix, "d-ragged-" + family, metric, rows, reqs, k, ids=ids)


# ------------------------------------------------------------------ counts
def test_per_request_k_k_above_the_eligible_rows_no_ranks_and_an_empty_batch(vdb):
    rows, _, reqs, _ = dd.ragged()
    n = len(rows)
    ks = np.array([1 + (37 * b) % 90 for b in range(len(reqs))])
    ks[3] = 0
    for metric in (dd.EUCLID, dd.COSINE):
        ix = make_index(vdb, metric, rows)
        got = check_routes(ix, "d-ragged-ks", metric, rows, reqs, ks)
        for (gi, _, _), kb in zip(got, ks):
            assert len(gi) == kb
        # k above len: every eligible row of every request, in order -- short lists, not an error
        full = check_routes(ix, "d-ragged-all", metric, rows, reqs, 5000)
        assert [len(gi) for gi, _, _ in full] == [n - len(set(dd.examples(r))) for r in reqs]
        # out_ranks = NULL: everything else is the same
        for route in ROUTES:
            gi, gd, gr, gc = run(ix, reqs, ks, route=route, want_ranks=False)
            assert gr is None
            for b, (x, y, _) in enumerate(got):
                assert int(gc[b]) == len(x) and same((gi[b, :len(x)], gd[b, :len(x)]), (x, y)), (metric, route, b)
    ix = make_index(vdb, dd.EUCLID, rows)
    gi, gd, gr, gc = ix.discover_batch([], [], 5)
    assert gc.size == 0 and ix.discover_stats() == [0] * 8
    gi, gd, gr, gc = ix.discover_batch([1], [[(2, 3)]], 0)
    assert gc.tolist() == [0]
    big = make_index(vdb, dd.EUCLID, bd.scaled(1500, 8))
    with pytest.raises(vdb.VectorDbError) as e:                                # more rows per request than the call returns
        big.discover_batch([1], [[]], 1025)
    assert "at most 1024" in str(e.value)
    assert big.discover_batch([1], [[(2, 3)]], 1024)[3].tolist() == [1024]


# ------------------------------------------------------------------ the two differential consequences
@pytest.mark.parametrize("metric", dd.METRICS)
def test_no_pairs_is_search_by_id(vdb, metric):
    sel = bd.spaced(bd.N, 24)
    ix = scaled_index(vdb, metric)
    reqs = [(int(r), ()) for r in sel]
    want = ix.search_batch_by_id(sel.astype(U64), bd.K)
    ok = (np.arange(bd.N) % 2) == 0
    mask, bits = id_mask(np.nonzero(ok)[0], bd.N)
    want_m = ix.search_batch_by_id(sel.astype(U64), bd.K, id_mask=mask, mask_bits=bits)
    for route in ROUTES:
        gi, gd, gr, gc = run(ix, reqs, bd.K, route=route)
        assert same((gi, gd, gc), want), (metric, route)
        assert (gr == 0).all()
        gi, gd, gr, gc = run(ix, reqs, bd.K, route=route, id_mask=mask, mask_bits=bits)
        assert same((gi, gd, gc), want_m), (metric, route, "masked")


@pytest.mark.parametrize("metric", dd.METRICS)
def test_one_pair_around_the_target_is_recommend_by_best_score(vdb, metric):
    """t = p, one pair (p, n), k = len: the rank-1 prefix is recommend_best_batch([p], [n]) with k = len, ids and dp bits"""
    rows, _, _, _ = dd.ragged()
    n = len(rows)
    ix = make_index(vdb, metric, rows)
    for p, ng in ((17, 301), (0, 1), (599, 44)):
        bi, bdp, _, bc = ix.recommend_best_batch([[p]], [[ng]], n)
        c = int(bc[0])
        assert 0 < c < n - 2
        for route in ROUTES:
            gi, gd, gr, gc = run(ix, [(p, ((p, ng),))], n, route=route)
            assert int(gc[0]) == n - 2
            assert (gr[0, :c] == 1).all() and (gr[0, c:n - 2] == 0).all()
            assert same((gi[0, :c], gd[0, :c]), (bi[0, :c], bdp[0, :c])), (metric, route, p, ng)


# ------------------------------------------------------------------ errors, in the order of the contract
def test_errors(vdb):
    n, d = 300, 16
    rows = bd.scaled(n, d).copy()
    ix = make_index(vdb, dd.EUCLID, rows)
    # (1) before (3): too many pairs wins over an id that is not stored; so does the k limit
    with pytest.raises(vdb.VectorDbError) as e:
        ix.discover_batch([900], [[(1, 2)] * 17], 3)
    assert "more than 16" in str(e.value)
    big = make_index(vdb, dd.EUCLID, bd.scaled(1500, 8))
    with pytest.raises(vdb.VectorDbError) as e:
        big.discover_batch([99999], [[]], 1025)
    assert "at most 1024" in str(e.value)
    # (2) staged writes are flushed: a row added a moment ago is a target, a removed one is not found
    ix.add(5000, vdb.Vector(rows[0] + F32(1)))
    assert ix.discover_batch([5000], [[(1, 2)]], 3)[3].tolist() == [3]
    ix.remove(5000)
    # (3) not found, in array order t, p_1, n_1, ... request by request
    for route in ROUTES:
        ix.debug_set_discover_route(route)
        with pytest.raises(vdb.VectorNotFound) as e:
            ix.discover_batch([1, 3], [[(2, 4), (777, 888)], [(999, 5)]], 3)
        assert e.value.id == 777
        with pytest.raises(vdb.VectorNotFound) as e:
            ix.discover_batch([1, 5000], [[(2, 4)], [(999, 5)]], 3)
        assert e.value.id == 5000
    ix.debug_set_discover_route(dd.AUTO)
    odd = np.ones(d + 3, dtype=F32)
    ix.add(7777, vdb.Vector(odd))
    with pytest.raises(vdb.DimensionMismatch) as e1:
        ix.recommend_batch([[7777, 1]], [[]], 3)
    with pytest.raises(vdb.DimensionMismatch) as e2:
        ix.discover_batch([7777], [[(1, 2)]], 3)
    assert (e2.value.expected, e2.value.actual) == (e1.value.expected, e1.value.actual)
    with pytest.raises(vdb.DimensionMismatch):
        ix.discover_batch([1], [[(5, 6)]], 3)
    ix.remove(7777)
    assert ix.discover_batch([1], [[(5, 6)]], 3)[3].tolist() == [3]
    # (4) Cosine: a zero-norm example (the target included), like any live zero-norm row, is an invalid vector on every route
    zrows = rows.copy()
    zrows[9] = 0
    cz = make_index(vdb, dd.COSINE, zrows)
    for route in ROUTES:
        for req in ((9, ()), (1, ((9, 2),)), (1, ((2, 9),)), (1, ((2, 3),))):
            with pytest.raises(vdb.InvalidVector):
                run(cz, [req], 3, route=route)
    cz.remove(9)
    want = dd.definition("d-zero-removed", dd.COSINE, zrows, [(1, ((2, 3),))], 3, live=(np.arange(n) != 9).astype(np.uint8))
    for route in ROUTES:
        dd.check(run(cz, [(1, ((2, 3),))], 3, route=route), want, route)
    with pytest.raises(ValueError):                                            # two pair lists for one target
        ix.discover_batch([1], [[(2, 3)], [(4, 5)]], 3)


def test_a_sharded_handle_is_refused_before_the_flush_and_the_ids(vdb):
    sh = make_index(vdb, dd.EUCLID, bd.scaled(3000, 16), devices=[0, 0])
    with pytest.raises(vdb.VectorDbError) as e:
        sh.discover_batch([1], [[(2, 3)]], 3)
    assert "sharded" in str(e.value)
    with pytest.raises(vdb.VectorDbError) as e:                                # an id that is not stored: still the refusal
        sh.discover_batch([999999], [[(2, 3)]], 3)
    assert "sharded" in str(e.value) and not isinstance(e.value, vdb.VectorNotFound)
    for call in (sh.discover_stats, lambda: sh.debug_set_discover_route(1)):
        with pytest.raises(vdb.VectorDbError) as e:
            call()
        assert "sharded" in str(e.value)
    assert sh.search_batch_by_id(np.array([1], dtype=U64), 3)[2].tolist() == [3]   # (the search by id serves it)


# ------------------------------------------------------------------ the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_discover(vdb, device_filter):
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
    reqs = [(2, ((half + 3, 7), (half, 1))), (5, ()), (half + 1, ((8, 9),)), (11, ((14, n - 1), (17, 20), (23, half + 5))), (2, ((2, 3), (3, 3))),
            (n - 2, ((n - 3, 0),))]
    red = (np.arange(n) % 3) == 2
    for flt, mask in ((None, None), (F.Eq("color", "red"), red.astype(np.uint8))):
        got = st.discover_batch([(name(t), [(name(p), name(g)) for p, g in pairs]) for t, pairs in reqs], k, flt)
        want = dd.definition(("d-store", flt is not None), dd.EUCLID, rows, reqs, k, mask=mask)
        assert len(got) == len(reqs)
        for b in range(len(reqs)):
            res, ranks = got[b]
            assert [r.id for r in res] == [name(int(i)) for i in want[b][0]], b
            assert np.array_equal(np.array([r.distance for r in res], dtype=F32).view(np.uint32), want[b][1].view(np.uint32)), b
            assert ranks == want[b][2].tolist(), b
        one, ranks = st.discover(name(reqs[3][0]), [(name(p), name(g)) for p, g in reqs[3][1]], k, flt)
        assert [(r.id, r.distance) for r in one] == [(r.id, r.distance) for r in got[3][0]] and ranks == got[3][1]
    with pytest.raises(vdb.VectorNotFound):
        st.discover(name(0), [(name(1), "nobody")], k)

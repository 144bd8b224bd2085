"""The edges of f32 -- +-inf inside the top-k, -0.0, subnormals, the Cosine denominator and its clamp, hidden NaN / zero-norm rows
-- through the five read kinds that came after tests/test_gpu_value_edges.py: search by stored id, recommend, one row per group,
a filter per query, MMR.  The families are tests/value_families.py; tests/test_value_edges_cpu.py proves what the oracle and the
models answer for each at the shapes used here (which stored rows are answered as queries, which folds are errors, which stage a
distinct search ends in, which MMR scores are NaN, infinite or subnormal).

Every comparison is on ids, order, counts and distance BITS (for MMR also score bits, with mmr_data.check's one liberty: any NaN
equals any NaN) against the expectation the existing models build from the CPU oracle (tests/value_edge_reads.py).  Where the
oracle errors the engine must raise the same class with the message of ERRORS, on every route.  No tolerance anywhere."""
import numpy as np
import pytest

import oracle
import by_id_data as bd
import distinct_data as dd
import mmr_data as md
import recommend_data as rd
import value_edge_reads as ver
import value_families as vf
from conftest import load_package
from test_gpu_mmr import raw_mmr
from test_gpu_value_edges import ERRORS, expect_error, same, with_tiers

pytestmark = pytest.mark.gpu

U64, F32 = np.uint64, np.float32
ROW_SHAPES = ("direct", "tiered", "screened")                      # by id and recommend: the rows become queries of the bf16 screening tier too
_IX = {}
_TABLES = {}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    yield v
    _IX.clear()
    for t in _TABLES.values():
        t.close()
    _TABLES.clear()


def build_index(vdb, metric, rows, dead, **ctor):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **ctor)
    ix.add_bulk(rows)
    for r in dead:
        ix.remove(int(r))
    return ix


def index_of(vdb, case, shape, hide=True, cache=True, **ctor):
    """(index, rows, queries, n): ids are the row numbers, dead_rows(n, hide) are tombstoned"""
    rows, q, n, _, _ = ver.case_data(case, shape)
    key = (ver.case_key(case, shape), hide, repr(sorted(ctor.items())))
    if key in _IX:
        return _IX[key], rows, q, n
    ix = build_index(vdb, case[1], rows, vf.dead_rows(n, hide), **ctor)
    if cache:
        if len(_IX) > 6:
            _IX.pop(next(iter(_IX)))
        _IX[key] = ix
    return ix, rows, q, n


def half_mask(vdb, n):
    """(on, words, compiled-mask factory) of id_mask(n, 0.5): the host mask and its twin compiled on the device"""
    on, words = vf.id_mask(n, 0.5, 7)
    if n not in _TABLES:
        t = vdb.MetaTable(0)
        t.set_codes(0, 0, on.astype(np.int32))
        t.set_present(0, n, True)
        _TABLES[n] = t
    return on, words, lambda: _TABLES[n].compile([(vdb.MetaTable.EQ, 0, 1)], n)


def raises(vdb, name, call, first=None):
    """the oracle's error: the same class, and one message on every route"""
    with pytest.raises(getattr(vdb, name)) as e:
        call()
    assert ERRORS[name] in str(e.value), str(e.value)
    assert first is None or str(e.value) == first, (str(e.value), first)
    return str(e.value)


def mixed_ks(count):
    return np.array([(10, 1, 64, 0)[i % 4] for i in range(count)], dtype=np.uintp)


# ================================================================== 1. search by stored id
def by_id_round(vdb, ix, case, shape, ids, live, tag, **mask):
    """the answered ids in one batch with per-query ks against the model and by_id_stats(); up to three refused ids alone and
    inside the good batch.  Returns the batch's arrays (None when the oracle answers fewer than 12 ids)."""
    good, at_kmax, bad = ver.by_id_split(case, shape, ids, 64, live, tag=tag)
    got = st = None
    if len(good) >= 12:
        ks = mixed_ks(len(good))
        _, want, _ = ver.by_id_split(case, shape, ids, ks, live, tag=tag)
        got = ix.search_batch_by_id(good.astype(U64), ks, **mask)
        st = ix.last_stats()
        bd.check(got, want, (case, shape, tag))
        assert ix.by_id_stats() == ver.by_id_stats(at_kmax), (case, shape, tag)
    else:
        assert case[0] == "inf_tail" and not case[2], (case, len(good))                  # only the plain inf_tail has nobody to answer
    msg = None
    for r, err in bad[:3]:
        msg = raises(vdb, err, lambda: ix.search_batch_by_id(np.array([r], dtype=U64), ver.K, **mask), msg)
        if len(good):
            raises(vdb, err, lambda: ix.search_batch_by_id(np.concatenate([good[:12], [r]]).astype(U64), ver.K, **mask), msg)
    return good, got, st


@pytest.mark.parametrize("shape", ROW_SHAPES)
@pytest.mark.parametrize("case", vf.ROW_QUERY_CASES, ids=vf.ROW_QUERY_IDS)
def test_by_id(vdb, case, shape):
    ix, rows, q, n = index_of(vdb, case, shape)
    live = vf.live_bytes(n)
    ids = vf.by_id_ids(n) if shape != "screened" else vf.by_id_ids(n)[:24]              # (the oracle is the slow side at 65536 rows)
    good, got, st = by_id_round(vdb, ix, case, shape, ids, live, "plain")
    if st is not None:
        assert st["bf16_screen"] == (1 if shape == "screened" else 0), st
    # a tombstoned id is not a stored id, alone or among good ones
    for dead in (0, vf.HIDDEN(n)):
        with pytest.raises(vdb.VectorNotFound) as e:
            ix.search_batch_by_id(np.concatenate([good[:3], [dead]]).astype(U64), ver.K)
        assert e.value.id == dead
    # under the half mask: rows 1 and 5 are ineligible but still valid queries; the compiled twin
    on, words, compiled = half_mask(vdb, n)
    mgood, mgot, _ = by_id_round(vdb, ix, case, shape, ids, live & on, "half", id_mask=words, mask_bits=n)
    if mgot is not None:
        with compiled() as cm:
            twin = ix.search_batch_by_id(mgood.astype(U64), mixed_ks(len(mgood)), compiled_mask=cm)
        assert same(mgot, twin), (case, shape)
    # the direct path of a small batch, and the same index without it
    if shape == "direct" and len(good):
        few = good[:5]
        want = ver.by_id_split(case, shape, ids, ver.K, live)[1][:5]
        a = ix.search_batch_by_id(few.astype(U64), ver.K)
        bd.check(a, want, (case, "direct path"))
        b = with_tiers(ix, ix.TIERS_NO_DIRECT, lambda: ix.search_batch_by_id(few.astype(U64), ver.K))
        assert same(a, b), case
        if got is not None:
            c = with_tiers(ix, ix.TIERS_NO_DIRECT, lambda: ix.search_batch_by_id(good.astype(U64), mixed_ks(len(good))))
            assert same(got, c), case


SHARDED_CASES = [c for c in vf.ROW_QUERY_CASES if c[0] in ("inf_tail", "overflow") and c[1] != vf.COSINE and (c[0] != "inf_tail" or c[2])]


@pytest.mark.parametrize("case", SHARDED_CASES, ids=["%s-m%d" % c[:2] for c in SHARDED_CASES])
def test_by_id_on_a_sharded_handle_strikes_after_the_merge(vdb, case):
    """the tie group at -inf / +inf spans the three shards: the merged k + 1 list is ordered by id, then the strike runs"""
    shape = "tiered"
    sh, rows, q, n = index_of(vdb, case, shape, cache=False, devices=[0, 0, 0])
    assert sh.shards() == 3
    live = vf.live_bytes(n)
    good, got, _ = by_id_round(vdb, sh, case, shape, vf.by_id_ids(n), live, "plain")
    plain, _, _, _ = index_of(vdb, case, shape)
    assert same(got, plain.search_batch_by_id(good.astype(U64), mixed_ks(len(good))))
    # the tie group at the head of a list has more than k members in EVERY shard: each shard's part is cut inside it
    bounds = np.cumsum([0] + [sh.shard_len(g) for g in range(3)])
    r = next((int(x) for x, (oi, od) in zip(good, ver.by_id_lists(case, shape, good, ver.K, live)) if od.view(np.uint32)[1] == od.view(np.uint32)[-1]), None)
    assert r is not None or case[:2] == ("inf_tail", vf.EUCLID)     # (there the rows that hold an inf are refused: the answered lists are finite)
    if r is not None:
        fi, fd = oracle.flat_search(case[1], rows, rows[r], n, live=live)
        tied = fi[fd.view(np.uint32) == fd.view(np.uint32)[ver.K]].astype(np.int64)
        assert all(((tied >= bounds[g]) & (tied < bounds[g + 1])).sum() > ver.K for g in range(3)), (case, r, len(tied))


# ================================================================== 2. recommend
def recommend(ix, reqs, k, **kw):
    pos, neg = rd.split(reqs)
    return ix.recommend_batch(pos, neg, k, **kw)


def recommend_round(vdb, ix, metric, rows, reqs, live, key, n_stored):
    """the requests the oracle answers in one batch against the model and recommend_stats(); up to three refused ones alone and
    inside the good batch"""
    good, want, bad = ver.recommend_split(metric, rows, reqs, ver.K, live, key)
    got = None
    if good:
        got = recommend(ix, good, ver.K)
        rd.check(got, want, key)
        assert ix.recommend_stats() == rd.stats(metric, rows, good, ver.K, n_stored, live=live), key
    msg = None
    for req, err in bad[:3]:
        msg = raises(vdb, err, lambda: recommend(ix, [req], ver.K), msg)
        if good:
            raises(vdb, err, lambda: recommend(ix, good + [req], ver.K), msg)
    return good, got, bad


@pytest.mark.parametrize("metric", vf.ALL)
@pytest.mark.parametrize("d", [33, 32])
def test_recommend_fold_edges(vdb, d, metric):
    """subnormal sums and averages, -0.0, a fold that overflows although its average is finite, inf - inf, FLT_MAX * rp and a
    fold whose norm underflows to 0: d = 33 takes the scalar loads, d = 32 the 16-byte ones"""
    rows, reqs = vf.fold_edges(d)
    names = [r[0] for r in vf.FOLD_REQUESTS]
    live = vf.live_bytes(vf.FOLD_N)
    ix = build_index(vdb, metric, rows, vf.dead_rows(vf.FOLD_N))
    good, got, bad = recommend_round(vdb, ix, metric, rows, reqs, live, ("fold_edges", d), int(live.sum()))
    assert {names[reqs.index(r)]: e for r, e in bad} == {nm: e[metric] for nm, e in vf.FOLD_ERRORS.items() if metric in e}
    # recommend == search with the numpy fold at k + m, struck on the host: the fold's BITS reach the search
    deep = ver.K + max(len(p) + len(x) for p, x in good)
    ai, ad, ac = ix.search_batch_arrays(rd.queries(rows, good), deep)
    for b, (p, x) in enumerate(good):
        m = ver.K + len(p) + len(x)
        si, sd = rd.strike(ai[b, :min(m, int(ac[b]))], ad[b, :min(m, int(ac[b]))], list(p) + list(x), ver.K)
        c = int(got[2][b])
        assert c == len(si) and np.array_equal(got[0][b, :c], si) and np.array_equal(got[1][b, :c].view(np.uint32), sd.view(np.uint32)), b
    with pytest.raises(vdb.VectorNotFound) as e:                                         # a tombstoned example
        recommend(ix, [good[0], ((40, 2), (41,))], ver.K)
    assert e.value.id == 2
    few = good[:5]                                                                      # the direct path of a small batch and without it
    a = recommend(ix, few, ver.K)
    assert same(a, with_tiers(ix, ix.TIERS_NO_DIRECT, lambda: recommend(ix, few, ver.K)))
    rd.check(a, rd.expected(metric, rows, few, ver.K, live=live), "few")


@pytest.mark.parametrize("shape", ROW_SHAPES)
@pytest.mark.parametrize("case", vf.ROW_QUERY_CASES, ids=vf.ROW_QUERY_IDS)
def test_recommend_from_rows_of_the_families(vdb, case, shape):
    ix, rows, q, n = index_of(vdb, case, shape)
    live = vf.live_bytes(n)
    good, got, bad = recommend_round(vdb, ix, case[1], rows, vf.row_requests(n), live, ver.case_key(case, shape), int(live.sum()))
    assert len(good) + len(bad) == 12
    if case[0] == "inf_tail" and not case[2]:
        assert not good
    else:
        assert good
        with pytest.raises(vdb.VectorNotFound) as e:
            recommend(ix, [good[0], ((1, 3), (n - 1,))], ver.K)
        assert e.value.id == n - 1


@pytest.mark.parametrize("metric", [vf.EUCLID, vf.DOT])
def test_recommend_fold_edges_on_a_sharded_handle(vdb, metric):
    """the examples of a request live on three shards; the fold order is the request's list order wherever the rows live"""
    rows, reqs = vf.fold_edges(33)
    live = vf.live_bytes(vf.FOLD_N)
    sh = build_index(vdb, metric, rows, vf.dead_rows(vf.FOLD_N), devices=[0, 0, 0])
    assert sh.shards() == 3 and all(sh.shard_len(g) > 0 for g in range(3))
    bounds = np.cumsum([0] + [sh.shard_len(g) for g in range(3)])
    assert any(len({int(np.searchsorted(bounds, r, side="right")) for r in p + x}) == 3 for p, x in reqs)
    good, got, bad = recommend_round(vdb, sh, metric, rows, reqs, live, ("fold_edges", 33), int(live.sum()))
    plain = build_index(vdb, metric, rows, vf.dead_rows(vf.FOLD_N))
    assert same(got, recommend(plain, good, ver.K))


# ================================================================== 3. one nearest row per group
def code_table(vdb, codes, n):
    t = vdb.MetaTable(0)
    t.set_codes(0, 0, np.ascontiguousarray(codes, dtype=np.int32))
    t.set_present(0, n, True)
    return t


def distinct_round(ix, table, case, shape, q, codes, live, tag, **mask):
    nq = len(q)
    length = int(vf.live_bytes(len(codes)).sum())
    ranks = [ver.ranking(case, shape, b, live, tag) for b in range(nq)]
    for stage, k in vf.DISTINCT_KS.items():
        gi, gd, gcodes, gn = ix.search_batch_distinct(q, k, table, 0, **mask)
        st = ix.distinct_stats()
        stages = [dd.stage_of(r, codes, k, length) for r in ranks]
        for b, rank in enumerate(ranks):
            ei, ed, ec = dd.expected(rank, codes, k)
            c = int(gn[b])
            what = (case, shape, tag, stage, b, stages[b])
            assert c == len(ei), what + (c, len(ei))
            assert np.array_equal(gi[b, :c], ei), what + (gi[b, :c], ei)
            assert np.array_equal(gd[b, :c].view(np.uint32), ed.view(np.uint32)), what + (gd[b, :c], ed)
            assert np.array_equal(gcodes[b, :c], ec), what
        assert st[:4] == [nq, stages.count("A"), stages.count("B"), stages.count("C")], (case, shape, tag, stage, st, stages)
        assert st[4] >= stages.count("C") and st[7] == int(gn.sum())
        if tag == "live":
            assert stages[0] == stage, (case, shape, stage, stages)                      # what tests/test_value_edges_cpu.py predicted


@pytest.mark.parametrize("shape", vf.READ_SHAPES)
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_distinct(vdb, family, metric, shape):
    case = ver.plain_case(family, metric)
    ix, rows, q, n = index_of(vdb, case, shape)
    d, nq = rows.shape[1], len(q)
    live = vf.live_bytes(n)
    codes = vf.distinct_codes(family, metric, n, d, nq)
    table = code_table(vdb, codes, n)
    try:
        distinct_round(ix, table, case, shape, q, codes, live, "live")
        on, words, _ = half_mask(vdb, n)
        distinct_round(ix, table, case, shape, q, codes, live & on, "half", id_mask=words, mask_bits=n)
        if vf.FAMILIES[family][2]:
            bad, _, _, _ = index_of(vdb, case, shape, hide=False)
            msg = expect_error(vdb, family, lambda: bad.search_batch_distinct(q, vf.DISTINCT_KS["A"], table, 0))
            expect_error(vdb, family, lambda: bad.search_batch_distinct(q, vf.DISTINCT_KS["C"], table, 0), msg)
    finally:
        table.close()


# ================================================================== 4. one batch, a filter per query
def grouped_ks(nq):
    return np.array([(10, 7, 1, 3)[(b // 5 + b) % 4] for b in range(nq)], dtype=np.uintp)


def check_grouped(got, metric, rows, qs, ks, go, on, live, what):
    gi, gd, gc = got
    for b in range(len(qs)):
        elig = live if go[b] == vf.GROUP_NONE else live & on[go[b]]
        oi, od = oracle.flat_search(metric, rows, qs[b], int(ks[b]), live=elig)
        c = int(gc[b])
        assert c == len(oi), what + (b, c, len(oi))
        assert np.array_equal(gi[b, :c], oi), what + (b, gi[b, :c], oi)
        assert np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), what + (b, gd[b, :c], od)


@pytest.mark.parametrize("shape", vf.READ_SHAPES)
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_grouped(vdb, family, metric, shape):
    case = ver.plain_case(family, metric)
    ix, rows, q, n = index_of(vdb, case, shape)
    live = vf.live_bytes(n)
    on, words, binding = vf.group_masks(n)
    qs = vf.group_queries(q)
    nq = len(qs)
    go, ks = binding(nq), grouped_ks(nq)
    short = go == 2
    assert (ks[short] > 6).any() and (ks[short] <= 6).any()                              # a k above the short mask's 6 eligible rows
    got = ix.search_batch_grouped(qs, 0, go, id_masks=words, mask_bits=n, ks=ks)
    st = ix.grouped_stats()
    check_grouped(got, metric, rows, qs, ks, go, on, live, (family, metric, shape))
    assert (got[2][short] == np.minimum(ks[short], 6)).all() and (got[2][go == 3] == 0).all()
    scanned = int(np.isin(go, (0, 1, 2)).sum())
    assert st[:5] == [nq, 4, scanned, 0, int((go == vf.GROUP_NONE).sum())] and st[6] > 0 and st[7] == 1, st
    error = vf.FAMILIES[family][2]
    if not error:
        return
    # the hidden row alive: only mask 0 and the unfiltered queries admit it
    bad, _, _, _ = index_of(vdb, case, shape, hide=False)
    on, words, _ = vf.group_masks(n, hide=False)
    alive = vf.live_bytes(n, hide=False)
    away = np.nonzero(~np.isin(go, (vf.GROUP_HOLDS_HIDDEN, vf.GROUP_NONE)))[0]
    call = lambda sel: bad.search_batch_grouped(qs[sel], 0, go[sel], id_masks=words, mask_bits=n, ks=ks[sel])
    if error == "InvalidVector":
        # include/vdb_flat.h: "under Cosine one live zero-norm row fails the call, masked or not" -- as the single masked search
        # does (tests/test_gpu_value_edges.py::test_masked_searches), which is what defines a query's answer
        msg = expect_error(vdb, family, lambda: call(away))
    else:
        check_grouped(call(away), metric, rows, qs[away], ks[away], go[away], on, alive, (family, metric, shape, "away"))
        msg = None
    for g in (vf.GROUP_HOLDS_HIDDEN, vf.GROUP_NONE):
        one = np.nonzero(go == g)[0][:1]
        msg = expect_error(vdb, family, lambda: call(np.sort(np.concatenate([away, one]))), msg)
        expect_error(vdb, family, lambda: call(one), msg)


# ================================================================== 5. MMR
def mmr_errors(vdb, ix, qs, k, m, lam, what, **mask):
    """a NaN pair among those evaluated: VDB_ERR_NAN from the C entry point and the Python exception"""
    if not mask:
        lams = None if np.isscalar(lam) else lam
        rc, _, _, _, _ = raw_mmr(vdb, ix, qs, k if np.isscalar(k) else 0, m, lam if np.isscalar(lam) else 0.0,
                                 ks=None if np.isscalar(k) else k, lams=lams)
        assert rc == vdb._ffi.ERR_NAN, what + (rc, vdb._ffi.last_error())
    with pytest.raises(vdb.NanDistance):
        ix.search_batch_mmr(qs, k if np.isscalar(k) else 0, m, lam, ks=None if np.isscalar(k) else k, **mask)


def mmr_round(vdb, ix, case, shape, qsel, k, m, lam, live, tag, stored=None, **mask):
    """one call against the model: the picks, distance and score bits and mmr_stats(), or VDB_ERR_NAN where the model evaluates
    a NaN pair for any query of the batch.  Returns (model, arrays or None)."""
    qs = np.ascontiguousarray(ver.case_data(case, shape)[1][list(qsel)])
    want = ver.mmr_want(case, shape, qsel, k, m, lam, live, stored=stored, tag=tag)
    what = (case, shape, tag, m, str(lam))
    if any(w["nan"] for w in want):
        mmr_errors(vdb, ix, qs, k, m, lam, what, **mask)
        return want, None
    got = ix.search_batch_mmr(qs, k if np.isscalar(k) else 0, m, lam, ks=None if np.isscalar(k) else k, **mask)
    md.check(got, want, what)
    assert ix.mmr_stats()[:5] == md.stats(want, m), (what, ix.mmr_stats(), md.stats(want, m))
    return want, got


@pytest.mark.parametrize("shape", vf.READ_SHAPES)
@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_mmr(vdb, family, metric, shape):
    case = ver.plain_case(family, metric)
    ix, rows, q, n = index_of(vdb, case, shape)
    nq = len(q)
    live = vf.live_bytes(n)
    qsel = tuple(range(nq))
    failed = False
    for lam in ver.LAMBDAS:
        want, got = mmr_round(vdb, ix, case, shape, qsel, ver.MMR_K, ver.MMR_M, lam, live, "plain")
        failed = failed or got is None
        if lam == 1.0 and got is not None:                          # the plain order exactly where the model says so
            pi, pd, pc = ix.search_batch_arrays(q, ver.MMR_K)
            for b, w in enumerate(want):
                equal = np.array_equal(got[0][b], pi[b]) and np.array_equal(got[1][b].view(np.uint32), pd[b].view(np.uint32))
                assert equal == (w["picks"] == list(range(len(w["picks"])))), (family, metric, shape, b, w["picks"])
    lams, ks = md.mixed(nq)
    want, got = mmr_round(vdb, ix, case, shape, qsel, ks, ver.MMR_M, lams, live, "plain")
    failed = failed or got is None
    # after an error the handle answers the next call: k = 1 evaluates no pair
    if failed:
        w1, g1 = mmr_round(vdb, ix, case, shape, qsel, 1, ver.MMR_M, 0.5, live, "plain")
        assert g1 is not None and ix.mmr_stats()[3] == 0
    assert failed == ((family, metric) in (("inf_tail", vf.EUCLID), ("inf_tail", vf.DOT), ("overflow", vf.COSINE), ("bf16_edge", vf.COSINE)))
    # under the half mask, with the compiled twin
    on, words, compiled = half_mask(vdb, n)
    want, got = mmr_round(vdb, ix, case, shape, qsel, ver.MMR_K, ver.MMR_M, 0.5, live & on, "half", stored=live, id_mask=words, mask_bits=n)
    with compiled() as cm:
        if got is None:
            with pytest.raises(vdb.NanDistance):
                ix.search_batch_mmr(q, ver.MMR_K, ver.MMR_M, 0.5, compiled_mask=cm)
        else:
            twin = ix.search_batch_mmr(q, ver.MMR_K, ver.MMR_M, 0.5, compiled_mask=cm)
            md.check(twin, want, (family, metric, shape, "compiled"))
            assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(got, twin))


@pytest.mark.parametrize("family,metric", vf.CASES, ids=vf.CASE_IDS)
def test_mmr_at_the_deepest_candidate_list(vdb, family, metric):
    """m = 1024, k = 16 on the tiered shape: every LDS entry in use, the tie groups of the families reach far into the list"""
    case = ver.plain_case(family, metric)
    shape = "tiered"
    ix, rows, q, n = index_of(vdb, case, shape)
    qsel = tuple(vf.checked_queries(len(q)))
    mmr_round(vdb, ix, case, shape, qsel, 16, 1024, 0.5, vf.live_bytes(n), "plain")

"""Exact range search (vdb_flat_range_search_batch) on every route: the screened route (score cut, filter pass,
every key re-ranked), the exact range scan and the dense fallback.  The expected answer of every case is the oracle's full
ranking cut at d <= r (tests/range_data.py; tests/test_range_cpu.py proves what the data is assumed to do): ids, order,
distance BITS, counts and totals are compared."""
import numpy as np
import pytest

import range_data as rd
import value_families as vf
from conftest import load_package

pytestmark = pytest.mark.gpu

F32 = np.float32
METRICS = (rd.EUCLID, rd.COSINE, rd.DOT)
ROUTE0, ROUTE1, ROUTE2 = 0, 1, 2


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def make(vdb, metric, rows, ids=None, devices=None):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, devices=devices)
    ix.add_bulk(rows, ids=ids)
    return ix


def check(ix, key, metric, rows, q, radii, mr, ids=None, live=None, mask=None, qsel=None):
    """One call; every query (or qsel) against the oracle's ranking `key` cut at its radius.  Returns (result, range_stats)."""
    radii_q = np.full(len(q), radii, dtype=F32) if np.isscalar(radii) else np.asarray(radii, dtype=F32)
    kw = {} if mask is None else {"id_mask": mask[0], "mask_bits": mask[1]}
    res = ix.range_search_batch(q, radii if np.isscalar(radii) else radii_q, mr, **kw)
    gi, gd, gc, gt = res
    st = ix.range_stats()
    assert st[ROUTE0] + st[ROUTE1] + st[ROUTE2] == len(q), st
    for b in (range(len(q)) if qsel is None else qsel):
        oi, od, c, total = rd.cut(rd.ranking((key, b), metric, rows, q[b], ids=ids, live=live), radii_q[b], mr)
        assert (int(gc[b]), int(gt[b])) == (c, total), (key, metric, b, float(radii_q[b]), int(gc[b]), int(gt[b]), c, total, st)
        assert np.array_equal(gi[b, :c], oi), (key, metric, b)
        assert np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), (key, metric, b)
    return res, st


def same(a, b):
    """two results equal in everything a caller may read: counts, totals and the written prefix of every row"""
    if not (np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])):
        return False
    return all(np.array_equal(a[0][i, :c], b[0][i, :c]) and np.array_equal(a[1][i, :c].view(np.uint32), b[1][i, :c].view(np.uint32))
               for i, c in enumerate(int(x) for x in a[2]))


# ------------------------------------------------------------------ 1. the screened route and where it hands over
@pytest.mark.parametrize("metric", METRICS)
def test_separated_family_routes(vdb, metric):
    rows, q, members = rd.separated()
    ix = make(vdb, metric, rows)
    r = rd.ENCLOSE[metric]
    # clusters of at most 300 rows: the gap makes the candidate list certain, every query ends on the screened route
    small = [b for b in range(rd.NQ) if rd.CLUSTERS[b % 4] <= 300]
    res, st = ix.range_search_batch(q[small], r, 512), ix.range_stats()
    assert st[ROUTE0] == len(small) and st[ROUTE1] == 0 and st[ROUTE2] == 0, st
    assert st[3] == rd.N and st[5] == 0 and st[6] == 0, st
    for i, b in enumerate(small):
        oi, od, c, total = rd.cut(rd.ranking(("sep", b), metric, rows, q[b]), r, 512)
        assert (int(res[2][i]), int(res[3][i])) == (c, total) == (rd.CLUSTERS[b % 4],) * 2
        assert np.array_equal(res[0][i, :c], oi) and np.array_equal(res[1][i, :c].view(np.uint32), od.view(np.uint32))
    # the whole batch: the 3000-row cluster has more than 2048 keys under any sound cut -> the exact range scan
    _, st = check(ix, "sep", metric, rows, q, r, 512)
    big = rd.NQ - len(small)
    assert (st[ROUTE0], st[ROUTE1], st[ROUTE2]) == (len(small), big, 0) and st[5] == big, st
    # a radius that encloses more than 32768 rows: the dense fallback
    rank0 = rd.ranking(("sep", 0), metric, rows, q[0])
    _, st = check(ix, "sep", metric, rows, q[:2], rd.radius_at(rank0, rd.DENSE_RANK), 2048, qsel=[0])
    assert st[ROUTE2] >= 1 and st[ROUTE0] == 0, st


@pytest.mark.parametrize("metric", METRICS)
def test_gaussian_rows_radii_at_neighbours(vdb, metric):
    rows, q = rd.gaussian()
    ix = make(vdb, metric, rows)
    left = 0
    for m in (1, 10, 200):
        radii = np.array([rd.radius_at(rd.ranking(("gauss", b), metric, rows, q[b]), m) for b in range(rd.NQ)], dtype=F32)
        _, st = check(ix, "gauss", metric, rows, q, radii, 256)
        left += st[ROUTE1] + st[ROUTE2]
        print(f"metric {metric} radius at neighbour {m}: range_stats {st}")
    print(f"metric {metric}: {left} of {3 * rd.NQ} queries left the screened route")


# ------------------------------------------------------------------ 2. radius edges
@pytest.mark.parametrize("metric", METRICS)
def test_radius_edges(vdb, metric):
    rows, q = rd.tied()
    ix = make(vdb, metric, rows)
    rank = rd.ranking(("tied", 0), metric, rows, q[0])
    r = rd.radius_at(rank, 1)
    (gi, gd, gc, gt), _ = check(ix, "tied", metric, rows, q, r, 16, qsel=[0])
    assert int(gt[0]) == len(rd.TIE_ROWS) and list(gi[0, :5]) == sorted(rd.TIE_ROWS)   # the whole group, ordered by id
    (gi, gd, gc, gt), _ = check(ix, "tied", metric, rows, q, rd.below(r), 16, qsel=[0])
    assert int(gt[0]) == 0 and int(gc[0]) == 0                                           # the whole group is out
    edges = [F32(-0.0), F32(np.inf), F32(0.0), F32(2.0), F32(-np.inf)]
    edges += [F32(-3.5)] if metric == rd.DOT else [F32(-1.0), F32(-1e-30)]
    for e in edges:
        (gi, gd, gc, gt), st = check(ix, "tied", metric, rows, q, e, 16)
        if metric != rd.DOT and e < 0:
            assert not gt.any() and not gc.any(), (e, gt)
        if e == F32(np.inf):
            assert (gt == rd.N).all() and st[ROUTE2] == len(q) and st[6] == len(q), st
    for bad_r, bad_mr in ((F32(np.nan), 8), (F32(1.0), 0), (F32(1.0), 2049)):
        with pytest.raises(vdb.VectorDbError) as e:
            ix.range_search_batch(q, bad_r, bad_mr)
        assert not isinstance(e.value, (vdb.NanDistance, vdb.InvalidVector, vdb.DimensionMismatch)), e.value
    with pytest.raises(vdb.VectorDbError):
        ix.range_search_batch(q, np.array([1.0, np.nan], dtype=F32), 8)
    ix.range_search_batch(q, F32(1.0), 2048)                                             # the largest max_results is served


# ------------------------------------------------------------------ 3. truncation
@pytest.mark.parametrize("metric", METRICS)
def test_truncation_counts_and_totals(vdb, metric):
    rows, q, members = rd.separated()
    ix = make(vdb, metric, rows)
    r = rd.ENCLOSE[metric]
    ranks = [rd.ranking(("sep", b), metric, rows, q[b]) for b in range(4)]
    # per query totals 1, 40, 300, 3000 under the enclosing radius; below, at and above every max_results
    for mr in (1, 7, 39, 40, 41, 2048):
        (gi, gd, gc, gt), _ = check(ix, "sep", metric, rows, q[:4], r, mr)
        assert list(gt) == list(rd.CLUSTERS) and list(gc) == [min(c, mr) for c in rd.CLUSTERS]
    # totals exactly max_results - 1, max_results, max_results + 1 for 1, 7 and 2048, from radii at those neighbours of query 3
    for mr in (1, 7, 2048):
        for m in (mr - 1, mr, mr + 1):
            if m == 0:
                radii = rd.below(rd.radius_at(ranks[3], 1))
            else:
                radii = rd.radius_at(ranks[3], m)
            (gi, gd, gc, gt), _ = check(ix, "sep", metric, rows, q[3:4], radii, mr, qsel=[])
            oi, od, c, total = rd.cut(ranks[3], radii, mr)
            assert (int(gc[0]), int(gt[0])) == (c, total) and total >= m and c == min(total, mr)
            assert np.array_equal(gi[0, :c], oi) and np.array_equal(gd[0, :c].view(np.uint32), od.view(np.uint32))


# ------------------------------------------------------------------ 4. per-query radii, two passes
def test_per_query_radii_in_a_batch_of_300(vdb):
    rows, q12, members = rd.separated()
    metric = rd.EUCLID
    ix = make(vdb, metric, rows)
    B = 300
    q = np.ascontiguousarray(q12[np.arange(B) % rd.NQ])
    ranks = [rd.ranking(("sep", b), metric, rows, q12[b]) for b in range(rd.NQ)]
    pick = [rd.ENCLOSE[metric], F32(-1.0), F32(0.0), rd.radius_at(ranks[1], 7), F32(1e-3), F32(30.0)]
    radii = np.array([pick[(b // rd.NQ) % len(pick)] for b in range(B)], dtype=F32)
    gi, gd, gc, gt = ix.range_search_batch(q, radii, 64)
    st = ix.range_stats()
    assert st[ROUTE0] + st[ROUTE1] + st[ROUTE2] == B and st[3] == 2 * rd.N, st
    for b in range(B):
        oi, od, c, total = rd.cut(ranks[b % rd.NQ], radii[b], 64)
        assert (int(gc[b]), int(gt[b])) == (c, total), (b, float(radii[b]))
        assert np.array_equal(gi[b, :c], oi) and np.array_equal(gd[b, :c].view(np.uint32), od.view(np.uint32)), b
    # a scalar radius and the same radius per query: identical output
    a = ix.range_search_batch(q, rd.ENCLOSE[metric], 64)
    b_ = ix.range_search_batch(q, np.full(B, rd.ENCLOSE[metric], dtype=F32), 64)
    assert same(a, b_) and np.array_equal(a[0], b_[0])


# ------------------------------------------------------------------ 5. masks, tombstones, upsert, compaction
def _bits(on):
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    return np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64), len(on)


@pytest.mark.parametrize("metric", METRICS)
def test_masks_tombstones_upsert_and_compaction(vdb, metric):
    rows0, q, members = rd.separated()
    rows = rows0.copy()
    ix = make(vdb, metric, rows)
    r = rd.ENCLOSE[metric]
    rng = np.random.default_rng(77 + metric)
    for sel, tag in ((0.10, "m10"), (0.001, "m01")):
        on = rng.random(rd.N) < sel
        on[members[1][::2]] = True                                   # half of the 40-row cluster stays eligible for certain
        _, st = check(ix, ("sep", tag), metric, rows, q[:4], r, 64, live=on.astype(np.uint8), mask=_bits(on))
    # removed rows: every third row of the 300-row cluster, a third of the 3000-row one, the single row
    dead = np.concatenate([members[2][::3], members[3][::3], members[0]])
    for i in dead:
        ix.remove(int(i))
    live = np.ones(rd.N, dtype=np.uint8)
    live[dead] = 0
    (gi, gd, gc, gt), st = check(ix, ("sep", "dead"), metric, rows, q[:4], r, 512, live=live)
    assert list(gt) == [0, 40, 200, 2000], gt
    # an upserted id: id of a background row moves into the single-row cluster's place
    up = int(np.setdiff1d(np.arange(100), np.concatenate(members))[0])
    ix.add(up, rows0[members[0][0]])
    rows[up] = rows0[members[0][0]]
    (gi, gd, gc, gt), st = check(ix, ("sep", "up"), metric, rows, q[:4], r, 512, live=live)
    assert int(gt[0]) == 1 and int(gi[0, 0]) == up
    before = ix.range_search_batch(q, r, 512)
    ix.compact()
    after = ix.range_search_batch(q, r, 512)
    assert same(before, after)
    check(ix, ("sep", "up"), metric, rows, q[:4], r, 512, live=live)


def test_zero_norm_row_behind_the_mask_fails_under_cosine(vdb):
    rows0, q, members = rd.separated()
    rows = rows0.copy()
    rows[12345] = 0.0
    ix = make(vdb, rd.COSINE, rows)
    on = np.ones(rd.N, dtype=bool)
    on[12345] = False
    m, bits = _bits(on)
    with pytest.raises(vdb.InvalidVector):
        ix.range_search_batch(q, rd.ENCLOSE[rd.COSINE], 8, id_mask=m, mask_bits=bits)
    with pytest.raises(vdb.InvalidVector):                           # a zero-norm query
        make(vdb, rd.COSINE, rows0).range_search_batch(np.zeros((1, rd.D), dtype=F32), F32(0.5), 8)
    with pytest.raises(vdb.DimensionMismatch):
        make(vdb, rd.EUCLID, rows0).range_search_batch(np.zeros((1, rd.D + 1), dtype=F32), F32(0.5), 8)
    empty = vdb.GpuFlatIndex(vdb.DistanceMetric(rd.EUCLID), keep_host_copy=False)
    gi, gd, gc, gt = empty.range_search_batch(np.zeros((2, 5), dtype=F32), F32(1.0), 8)
    assert not gc.any() and not gt.any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", ["screened", "tiered"])
def test_nan_hidden_row(vdb, metric, shape):
    """hidden (removed, or masked out): success; alive and eligible: VDB_ERR_NAN -- on the screened route and on the scan"""
    n, d, nq, _ = vf.SHAPES[shape]
    rows, q = vf.make("nan_hidden", n, d, nq, metric)
    q = q[:4]
    h = vf.HIDDEN(n)
    ix = make(vdb, metric, rows)
    with pytest.raises(vdb.NanDistance):
        ix.range_search_batch(q, F32(0.5) if metric != rd.DOT else F32(-1.0), 16)
    on = np.ones(n, dtype=bool)
    on[h] = False
    clean = np.where(np.isnan(rows), F32(0.0), rows)
    r = rd.radius_at(rd.ranking(("nanh", shape, 0), metric, clean, q[0], live=on.astype(np.uint8)), 5)
    check(ix, ("nanh", shape), metric, clean, q, r, 16, live=on.astype(np.uint8), mask=_bits(on))
    st = ix.range_stats()
    assert st[ROUTE1] == len(q) or shape == "screened", st
    ix.remove(h)
    check(ix, ("nanh", shape), metric, clean, q, r, 16, live=on.astype(np.uint8))


# ------------------------------------------------------------------ 6. small indexes and the screening tier switched off
@pytest.mark.parametrize("metric", METRICS)
def test_small_index_and_screen_off_take_the_scan(vdb, metric):
    rng = np.random.default_rng(900 + metric)
    for n, d in ((1000, 16), (20000, 48)):
        rows = rng.standard_normal((n, d)).astype(F32)
        q = (rows[rng.integers(0, n, 9)] + F32(0.05) * rng.standard_normal((9, d)).astype(F32)).astype(F32)
        ix = make(vdb, metric, rows)
        for m in (1, 30):
            radii = np.array([rd.radius_at(rd.ranking(("small", n, b), metric, rows, q[b]), m) for b in range(9)], dtype=F32)
            _, st = check(ix, ("small", n), metric, rows, q, radii, 64)
            assert (st[ROUTE0], st[ROUTE1], st[3]) == (0, 9, 0), st
    rows, q, members = rd.separated()
    ix = make(vdb, metric, rows)
    a, sa = check(ix, "sep", metric, rows, q, rd.ENCLOSE[metric], 512)
    ix.set_screen(0)
    b, sb = check(ix, "sep", metric, rows, q, rd.ENCLOSE[metric], 512)
    assert sa[ROUTE0] > 0 and (sb[ROUTE0], sb[ROUTE1], sb[3]) == (0, rd.NQ, 0), (sa, sb)
    assert same(a, b)


# ------------------------------------------------------------------ 7. value families on their boundary radii
RANGE_FAMILIES = [(f, m) for f in ("inf_tail", "overflow", "subnormal", "dot_zero", "cos_den_clamp") for m in vf.FAMILIES[f][1]]


@pytest.mark.parametrize("shape", ["direct", "screened"])
@pytest.mark.parametrize("family,metric", RANGE_FAMILIES, ids=["%s-m%d" % c for c in RANGE_FAMILIES])
def test_value_families_on_boundary_radii(vdb, family, metric, shape):
    n, d, nq, _ = vf.SHAPES[shape]
    rows, q = vf.make(family, n, d, nq, metric)
    q = q[vf.checked_queries(nq)]
    ix = make(vdb, metric, rows)
    for r in (F32(np.inf), F32(-np.inf), F32(0.0), F32(-0.0), F32(1.0), F32(2.0)):
        check(ix, (family, shape), metric, rows, q, r, 64)


# ------------------------------------------------------------------ 8. the device entry point
def test_device_entry_point_and_an_outstanding_ticket(vdb):
    import torch
    rows, q, members = rd.separated()
    metric = rd.EUCLID
    ix = make(vdb, metric, rows)
    rank0 = rd.ranking(("sep", 0), metric, rows, q[0])
    radii = np.full(rd.NQ, rd.ENCLOSE[metric], dtype=F32)
    radii[0] = rd.radius_at(rank0, rd.DENSE_RANK)                    # one query on the dense fallback, the 3000-row clusters on the scan
    mr = 64
    host = ix.range_search_batch(q, radii, mr)
    dev = torch.device("cuda", 0)
    q_t, r_t = torch.from_numpy(q.copy()).to(dev), torch.from_numpy(radii).to(dev)

    def outputs():
        return (torch.zeros((rd.NQ, mr), dtype=torch.int64, device=dev), torch.zeros((rd.NQ, mr), dtype=torch.float32, device=dev),
                torch.zeros((rd.NQ,), dtype=torch.int32, device=dev), torch.zeros((rd.NQ,), dtype=torch.int64, device=dev))

    def run(o):
        ix.range_search_batch_device(q_t.data_ptr(), rd.NQ, rd.D, r_t.data_ptr(), mr, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                                     out_totals_ptr=o[3].data_ptr())
        torch.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64), o[1].cpu().numpy(), o[2].cpu().numpy().astype(np.uint64),
                o[3].cpu().numpy().view(np.uint64))

    torch.cuda.synchronize()
    got = run(outputs())
    assert same(host, got)
    for b in range(rd.NQ):                                           # unused slots are padded: id 2^64 - 1, NaN distance
        c = int(got[2][b])
        assert (got[0][b, c:] == np.uint64(2**64 - 1)).all() and np.isnan(got[1][b, c:]).all()
    # totals may be omitted
    o = outputs()
    ix.range_search_batch_device(q_t.data_ptr(), rd.NQ, rd.D, r_t.data_ptr(), mr, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(o[2].cpu().numpy().astype(np.uint64), got[2]) and not o[3].cpu().numpy().any()
    # one submitted search outstanding: the device form runs in the other workspace, the host form is refused
    k = 10
    s_out = (torch.empty((rd.NQ, k), dtype=torch.int64, device=dev), torch.empty((rd.NQ, k), dtype=torch.float32, device=dev),
             torch.empty((rd.NQ,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ticket = ix.search_batch_device_submit(q_t.data_ptr(), rd.NQ, rd.D, k, s_out[0].data_ptr(), s_out[1].data_ptr(), s_out[2].data_ptr())
    try:
        again = run(outputs())
        with pytest.raises(vdb.VectorDbError):
            ix.range_search_batch(q, radii, mr)
    finally:
        ix.search_batch_device_wait(ticket)
    torch.cuda.synchronize()
    assert same(host, again)
    want = ix.search_batch_arrays(q, k)
    assert np.array_equal(s_out[0].cpu().numpy().view(np.uint64), want[0])


# ------------------------------------------------------------------ 9. a sharded handle, the store
def test_sharded_handle_is_refused(vdb):
    rows, q = rd.gaussian()
    sh = make(vdb, rd.EUCLID, rows[:4096], devices=[0, 0])
    with pytest.raises(vdb.VectorDbError) as e:
        sh.range_search_batch(q, F32(1.0), 8)
    assert "sharded" in str(e.value)
    with pytest.raises(vdb.VectorDbError):
        sh.range_stats()


def test_store_search_within(vdb):
    import oracle
    rng = np.random.default_rng(31)
    n, d = 3000, 24
    rows = rng.standard_normal((n, d)).astype(F32)
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    colours = ["red", "green", "blue"]
    for i in range(n):
        store.insert_with_metadata(f"v{i}", vdb.Vector(rows[i]), vdb.Metadata({"colour": colours[i % 3], "n": str(i % 7)}))
    store.delete("v10")
    q = (rows[10] + F32(0.01)).astype(F32)
    oi, od = oracle.flat_search(0, rows, q, n, live=(np.arange(n) != 10).astype(np.uint8))
    r = F32(od[49])
    got = store.search_within(vdb.Vector(q), r, 100)
    want = [(f"v{int(i)}", float(x)) for i, x in zip(oi, od) if x <= r]
    assert len(want) >= 50 and [(g.id, g.distance) for g in got] == want
    assert [(g.id, g.distance) for g in store.search_within(vdb.Vector(q), r, 7)] == want[:7]
    flt = vdb.MetadataFilter.And([vdb.MetadataFilter.Eq("colour", "green"), vdb.MetadataFilter.Ne("n", "3")])
    r2 = F32(od[999])
    got = store.search_within(vdb.Vector(q), r2, 2048, flt)
    want = [(f"v{int(i)}", float(x)) for i, x in zip(oi, od) if x <= r2 and int(i) % 3 == 1 and int(i) % 7 != 3]
    assert len(want) > 100 and [(g.id, g.distance) for g in got] == want
    assert store.search_within(vdb.Vector(q), F32(-1.0), 10) == []

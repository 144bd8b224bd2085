"""The sparse-filter route of pre-filtered flat searches (vdb_flat_set_sparse_filter, csrc/kernels_sparse.hip): under an id mask
only the eligible rows are scanned.  Every result is compared with the CPU oracle (ids, order, distance bits) AND with mode 0 on
the same handle (arrays identical); sparse_stats()[0] says which of the two really ran.

The first test exercises the eligible-row list alone (no scan kernel is launched by it): run it before the others."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu


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
    """(words, mask_bits) with the bits of `ids` set"""
    ids = np.asarray(ids, dtype=np.uint64)
    top = max(int(bits), int(ids.max()) + 1 if ids.size else 0)                  # bits may be set at or above mask_bits: they name nothing
    m = np.zeros((top + 63) // 64 + 1, dtype=np.uint64)
    if ids.size:
        np.bitwise_or.at(m, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return m, bits


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def check_oracle(metric, rows, q, k, res, qsel, ids=None, live=None):
    gi, gd, gc = res
    for b in qsel:
        oi, od = oracle.flat_search(metric, rows, q[b], k, ids=ids, live=live)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)


def both_modes(ix, q, k, mask, bits, expect_route=True):
    """(mode 1 results, mode 0 results); asserts through sparse_stats which path answered"""
    ix.set_sparse_filter(0)
    ref = ix.search_batch_arrays(q, k, id_mask=mask, mask_bits=bits)
    assert ix.sparse_stats()[0] == 0
    ix.set_sparse_filter(1)
    n_before = ix.sparse_stats()[2]
    got = ix.search_batch_arrays(q, k, id_mask=mask, mask_bits=bits)
    st = ix.sparse_stats()
    assert st[0] == (1 if expect_route else 0) and st[2] == n_before + (1 if expect_route else 0), st
    ix.set_sparse_filter(0)
    return got, ref


# ------------------------------------------------------------------ 1. the eligible-row list alone
def test_eligible_row_list_alone(vdb):
    rng = np.random.default_rng(1)
    n, d = 3000, 5
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(3)                    # non-monotone, with gaps; id 0 is stored
    ix = make_index(vdb, 0, rows, ids=ids)
    live = np.ones(n, dtype=bool)
    for r in range(0, n, 7):
        ix.remove(int(ids[r]))
        live[r] = False
    top = int(ids.max()) + 1

    def expect(mask, bits):
        ok = live & (ids < np.uint64(bits))
        w = mask[(ids[ok] >> np.uint64(6)).astype(np.int64)]
        sel = ((w >> (ids[ok] & np.uint64(63))) & np.uint64(1)).astype(bool)
        return np.nonzero(ok)[0][sel].astype(np.uint32)

    last_word = np.arange(n // 32 * 32, n)                                       # rows of the final partial 32-bit word (3000 = 93 * 32 + 24)
    assert 0 < last_word.size < 32
    cases = {
        "none": id_mask([], top),
        "bit 0 only": id_mask([0], top),
        "first row": id_mask([ids[1]], top),
        "last row": id_mask([ids[n - 1]], top),
        "final partial word": id_mask(ids[last_word], top),
        "all rows": id_mask(ids, top),
        "mask_bits below the ids": id_mask(ids, int(ids.max()) // 2),
        "mask_bits above the ids": id_mask(ids[::3], top + 5000),
        "ids that are not stored": id_mask(np.concatenate([ids[5:400], np.arange(1, top, 3, dtype=np.uint64)]), top),
        "all bits set": (np.full(top // 64 + 2, ~np.uint64(0), dtype=np.uint64), top),
    }
    n_route = ix.sparse_stats()[2]
    for name, (m, bits) in cases.items():
        got = ix.debug_eligible_rows(m, bits)
        want = expect(m, bits)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (name, got[:10], want[:10], got.size, want.size)
    assert expect(*cases["last row"]).tolist() == [n - 1] and expect(*cases["all rows"]).size == int(live.sum())
    assert expect(*cases["none"]).size == 0 and expect(*cases["bit 0 only"]).size == int(live[np.nonzero(ids == 0)[0][0]])
    assert np.array_equal(expect(*cases["ids that are not stored"]), expect(*id_mask(ids[5:400], top)))
    assert ix.sparse_stats()[2] == n_route                                       # no search was answered: nothing was scanned


# ------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", [1, 3, 33, 100])
def test_tile_edges(vdb, metric, d):
    tile_r, tile_q = vdb.GpuFlatIndex.sparse_tile()
    rng = np.random.default_rng(100 * metric + d)
    n = 4000
    rows = (rng.standard_normal((n, d)) + (0.5 if d == 1 else 0.0)).astype(np.float32)
    rows[rows == 0] = 1.0
    qall = rng.standard_normal((257, d)).astype(np.float32)
    ix = make_index(vdb, metric, rows)
    for E in (1, tile_r - 1, tile_r, tile_r + 1, 700):
        keep = np.sort(rng.choice(n, size=E, replace=False))
        live = np.zeros(n, dtype=np.uint8)
        live[keep] = 1
        m, bits = id_mask(keep, n)
        for nq in (1, 9, tile_q + 1, 257):
            q = qall[:nq]
            for k in sorted({1, 10, E, E + 3}):
                got, ref = both_modes(ix, q, k, m, bits)
                assert same(got, ref), (E, nq, k)
                assert ix.sparse_stats()[1] == E
                check_oracle(metric, rows, q, k, got, sorted({0, nq - 1}), live=live)
                assert (got[2] == min(k, E)).all()


# ------------------------------------------------------------------ 3. ties and ids
def test_ties_permuted_ids_overwrites_and_compaction(vdb):
    rng = np.random.default_rng(3)
    n, d, k = 2500, 12, 20
    base = rng.standard_normal((n // 5, d)).astype(np.float32)
    rows = np.tile(base, (5, 1))                                                 # every vector five times, under different ids
    ids = rng.permutation(n).astype(np.uint64) + np.uint64(10)                   # permuted: the id-rank path
    q = np.concatenate([base[:6] + np.float32(0.01), rng.standard_normal((5, d)).astype(np.float32)])
    for metric in (0, 1, 2):
        ix = make_index(vdb, metric, rows, ids=ids)
        all_rows, all_ids, live = rows.copy(), ids.copy(), np.ones(n, dtype=np.uint8)
        # an id added twice: the last one wins, the first row is dead
        again = np.array([3, 700, 2499])
        new_rows = rng.standard_normal((again.size, d)).astype(np.float32)
        ix.add_bulk(new_rows, ids=ids[again])
        live[again] = 0
        all_rows = np.concatenate([all_rows, new_rows]); all_ids = np.concatenate([all_ids, ids[again]])
        live = np.concatenate([live, np.ones(again.size, dtype=np.uint8)])
        keep = rng.random(all_ids.size) < 0.3
        keep[again] = True
        m, bits = id_mask(all_ids[keep], int(all_ids.max()) + 1)
        elig = live & np.isin(all_ids, all_ids[keep]).astype(np.uint8)
        got, ref = both_modes(ix, q, k, m, bits)
        assert same(got, ref)
        check_oracle(metric, all_rows, q, k, got, range(q.shape[0]), ids=all_ids, live=elig)
        n_tied = 0
        for b in range(q.shape[0]):                                              # equal distances come in ascending id order
            gd, gi = got[1][b, :got[2][b]], got[0][b, :got[2][b]]
            tied = np.nonzero(gd[1:].view(np.uint32) == gd[:-1].view(np.uint32))[0]
            assert (gi[tied + 1] > gi[tied]).all()
            n_tied += tied.size
        assert n_tied > 0
        assert ix.compact() == again.size
        got2, ref2 = both_modes(ix, q, k, m, bits)
        assert same(got2, ref2) and same(got2, got)


# ------------------------------------------------------------------ 4. the select's capacity
def test_k_2048_takes_the_route_and_2049_does_not(vdb):
    rng = np.random.default_rng(4)
    n, d, E = 9000, 16, 5000
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    ix = make_index(vdb, 0, rows)
    keep = np.sort(rng.choice(n, size=E, replace=False))
    live = np.zeros(n, dtype=np.uint8)
    live[keep] = 1
    m, bits = id_mask(keep, n)
    got, ref = both_modes(ix, q, 2048, m, bits, expect_route=True)
    assert same(got, ref) and (got[2] == 2048).all()
    check_oracle(0, rows, q, 2048, got, [0, 2], live=live)
    got, ref = both_modes(ix, q, 2049, m, bits, expect_route=False)
    assert same(got, ref) and (got[2] == 2049).all()
    check_oracle(0, rows, q, 2049, got, [1], live=live)


# ------------------------------------------------------------------ 5. errors
def test_error_semantics(vdb):
    rng = np.random.default_rng(5)
    n, d = 3000, 8
    rows = rng.random((n, d), dtype=np.float32) + np.float32(0.1)
    q = rng.random((4, d), dtype=np.float32) + np.float32(0.1)
    keep = np.arange(0, n, 11)
    m, bits = id_mask(keep, n + 10)
    c = make_index(vdb, 1, rows)
    qz = q.copy()
    qz[2] = 0.0
    for mode in (0, 1):
        c.set_sparse_filter(mode)
        with pytest.raises(vdb.InvalidVector):                                   # zero-norm query under Cosine
            c.search_batch_arrays(qz, 3, id_mask=m, mask_bits=bits)
        with pytest.raises(vdb.InvalidVector):                                   # ... also when nothing is eligible
            c.search_batch_arrays(qz, 3, id_mask=np.zeros_like(m), mask_bits=bits)
        with pytest.raises(vdb.DimensionMismatch):
            c.search_batch_arrays(q[:, :7], 3, id_mask=m, mask_bits=bits)
    got, ref = both_modes(c, q, 3, m, bits)
    assert same(got, ref)
    e = make_index(vdb, 0, rows)
    e.add(n, vdb.Vector([float("nan")] + [1.0] * (d - 1)))                       # id n: a NaN row
    m_in, _ = id_mask(np.concatenate([keep, [n]]), n + 10)
    for mode in (0, 1):
        e.set_sparse_filter(mode)
        with pytest.raises(vdb.VectorDbError):                                   # eligible: the reference panics (flat_index.rs:62)
            e.search_batch_arrays(q, 3, id_mask=m_in, mask_bits=bits)
    outcomes = []
    for mode in (0, 1):                                                          # masked out: the same outcome as mode 0
        e.set_sparse_filter(mode)
        try:
            outcomes.append(("ok", e.search_batch_arrays(q, 3, id_mask=m, mask_bits=bits)))
        except vdb.VectorDbError as err:
            outcomes.append(("error", type(err)))
    assert outcomes[0][0] == outcomes[1][0]
    if outcomes[0][0] == "ok":
        assert same(outcomes[0][1], outcomes[1][1])
        live = np.zeros(n, dtype=np.uint8)
        live[keep] = 1
        check_oracle(0, rows, q, 3, outcomes[1][1], range(4), live=live)
    else:
        assert outcomes[0][1] is outcomes[1][1]
    # nothing eligible, a search without a mask, an empty batch
    e.remove(n)
    e.set_sparse_filter(1)
    r = e.search_batch_arrays(q, 3, id_mask=np.zeros_like(m), mask_bits=bits)
    assert (r[2] == 0).all() and e.sparse_stats()[:2] == [1, 0]
    r = e.search_batch_arrays(q, 3)
    assert (r[2] == 3).all() and e.sparse_stats()[0] == 0


# ------------------------------------------------------------------ 6. an index on the screening tier
def test_screening_tier_index_at_two_selectivities(vdb):
    rng = np.random.default_rng(6)
    n, d, k = 70000, 8, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((40, d)).astype(np.float32)
    ix = make_index(vdb, 0, rows)
    for i in range(0, n, 9):
        ix.remove(i)
    for E in (700, 21):                                                          # 1 % and 0.03 %
        keep = np.sort(rng.choice(n, size=E, replace=False))
        live = np.zeros(n, dtype=np.uint8)
        live[keep] = 1
        live[::9] = 0
        m, bits = id_mask(keep, n)
        ix.set_sparse_filter(0)
        ref = ix.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
        assert ix.last_stats()["bf16_screen"] == 1 and ix.sparse_stats()[0] == 0
        got, ref2 = both_modes(ix, q, k, m, bits)
        assert same(got, ref) and same(ref, ref2)
        assert ix.sparse_stats()[1] == int(live.sum()) and ix.last_stats()["exact_queries"] == q.shape[0]
        check_oracle(0, rows, q, k, got, [0, 17, 39], live=live)


# ------------------------------------------------------------------ 7. two batches in flight
def test_submit_wait_in_mode_1(vdb):
    import torch
    rng = np.random.default_rng(7)
    n, d, B, k = 30000, 24, 70, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 2, rows)
    keep = np.sort(rng.choice(n, size=900, replace=False))
    m, bits = id_mask(keep, n)
    dev = torch.device("cuda", 0)
    qn = [rng.standard_normal((B, d)).astype(np.float32) for _ in range(2)]
    ix.set_sparse_filter(0)
    ref = [ix.search_batch_arrays(x, k, id_mask=m, mask_bits=bits) for x in qn]
    qs = [torch.from_numpy(x).to(dev) for x in qn]
    m_t = torch.from_numpy(m.view(np.int64)).to(dev)
    outs = [(torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
             torch.empty((B,), dtype=torch.int32, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    ix.set_sparse_filter(1)
    before = ix.sparse_stats()[2]
    t = [ix.search_batch_device_submit(qs[i].data_ptr(), B, d, k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), outs[i][2].data_ptr(),
                                       mask_ptr=m_t.data_ptr(), mask_bits=bits) for i in range(2)]
    for x in t:
        ix.search_batch_device_wait(x)
    torch.cuda.synchronize()
    assert ix.sparse_stats()[2] == before + 2 and ix.sparse_stats()[0] == 1
    for i in range(2):
        assert np.array_equal(outs[i][2].cpu().numpy(), ref[i][2].astype(np.int32)) and (ref[i][2] == k).all()
        assert np.array_equal(outs[i][0].cpu().numpy().view(np.uint64), ref[i][0])
        assert np.array_equal(outs[i][1].cpu().numpy().view(np.uint32), ref[i][1].view(np.uint32))


# ------------------------------------------------------------------ 8. a sharded handle
def test_sharded_handle_in_mode_1(vdb):
    rng = np.random.default_rng(8)
    n, d, B, k = 20000, 20, 33, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    keep = np.sort(rng.choice(n, size=400, replace=False))
    live = np.zeros(n, dtype=np.uint8)
    live[keep] = 1
    m, bits = id_mask(keep, n)
    plain = make_index(vdb, 1, rows)
    ref = plain.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
    sh = make_index(vdb, 1, rows, devices=[0, 0, 0])
    assert same(ref, sh.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)) and sh.sparse_stats()[0] == 0
    sh.set_sparse_filter(1)
    before = sh.sparse_stats()[2]
    got = sh.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
    st = sh.sparse_stats()
    assert st[0] == 1 and st[1] == keep.size and st[2] == before + 3, st          # every shard took the route, the lists add up
    assert same(ref, got)
    check_oracle(1, rows, q, k, got, [0, 16, 32], live=live)
    sh.set_sparse_filter(0)
    assert same(ref, sh.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)) and sh.sparse_stats()[0] == 0


# ------------------------------------------------------------------ 9. the automatic mode
def test_mode_2_follows_sparse_limit(vdb):
    rng = np.random.default_rng(9)
    n, d, k = 20000, 32, 5
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 0, rows)
    for nq in (1, 16, 64):
        q = rng.standard_normal((nq, d)).astype(np.float32)
        limit = vdb.GpuFlatIndex.sparse_limit(n, 32, d, nq)
        for E in sorted({0, 1, 50, limit, limit + 1, 3000}):
            if E > n:
                continue
            keep = np.sort(rng.choice(n, size=E, replace=False))
            live = np.zeros(n, dtype=np.uint8)
            live[keep] = 1
            m, bits = id_mask(keep, n)
            ix.set_sparse_filter(0)
            ref = ix.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
            ix.set_sparse_filter(2)
            got = ix.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
            st = ix.sparse_stats()
            assert st[1] == E and st[0] == (1 if E <= limit else 0), (nq, E, limit, st)
            assert same(got, ref)
            check_oracle(0, rows, q, k, got, [0, nq - 1], live=live)
    # a small index and a few queries keep the direct path in mode 2 (and lose it to the route in mode 1)
    small = make_index(vdb, 0, rows[:1000])
    m, bits = id_mask([], 1000)
    q = rng.standard_normal((2, d)).astype(np.float32)
    small.set_sparse_filter(2)
    r = small.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
    assert (r[2] == 0).all() and small.sparse_stats()[0] == 0
    small.set_sparse_filter(1)
    r = small.search_batch_arrays(q, k, id_mask=m, mask_bits=bits)
    assert (r[2] == 0).all() and small.sparse_stats()[0] == 1

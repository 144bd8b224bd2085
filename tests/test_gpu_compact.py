"""vdb_flat_compact on the GPU: the in-place stable compaction of the device row store changes no search result -- ids, order,
counts and distance BITS equal the result before it, a fresh index bulk-loaded with the survivors in the same order, and the
CPU oracle -- on every tier, with every opt-in path, on plain and sharded handles and through VectorStore; per-row state is
moved, not recomputed; the index goes on living afterwards."""
import numpy as np
import pytest

import lifecycle
import oracle
from conftest import load_package
from test_compact_cpu import pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def Model(vdb, metric, rows, ix=None, **kw):
    """What the device store must hold (lifecycle.Model: every row ever appended, in order, with its id and whether it is still
    alive), driving an index: every mutation of the model goes to the index too."""
    return lifecycle.Model.driving(vdb, metric, rows, ix=ix, **kw)


def same(a, b):
    return np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def churn(m, rng, remove_frac, overwrite_frac):
    n, d = m.rows.shape
    perm = rng.permutation(n)
    n_rm, n_ow = int(n * remove_frac), int(n * overwrite_frac)
    m.remove(m.ids[perm[:n_rm]])
    if n_ow:
        ow = np.sort(perm[n_rm:n_rm + n_ow])
        m.add_bulk(rng.standard_normal((n_ow, d)).astype(np.float32), m.ids[ow])


# ------------------------------------------------------------------ 1. results do not change, all tiers
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_results_do_not_change_on_any_tier(vdb, metric):
    rng = np.random.default_rng(100 + metric)
    n, d, nq = 100_000, 128, 64
    m = Model(vdb, metric, rng.standard_normal((n, d)).astype(np.float32))
    churn(m, rng, 0.30, 0.10)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ix, n_live = m.ix, 70_000
    assert ix.len() == n_live and ix.store_stats()[:2] == [n + 10_000, n_live]
    before = {k: ix.search_batch_arrays(q, k) for k in (1, 10, 100)}
    scanned = ix.last_stats()["rows_scanned"]
    assert scanned and scanned % (n + 10_000) == 0                   # dead rows are scanned too, until they are taken back
    assert m.compact() == 40_000
    st = ix.store_stats()
    assert st[0] == ix.len() == n_live and st[1] == n_live and st[4] == 1 and st[5] == 40_000 and st[6] > 0 and st[2] >= n + 10_000
    fresh = m.fresh()
    for k in (1, 10, 100):
        after = m.check(q, k, qsel=range(0, nq, 1 if k == 10 else 8))
        assert same(after, before[k]), k
        scanned = ix.last_stats()["rows_scanned"]
        assert same(after, fresh.search_batch_arrays(q, k)), k
        assert scanned and scanned % n_live == 0, (k, scanned)      # every pass over the rows now reads the live rows only
    for flags in (ix.TIERS_FORCE_F32, ix.TIERS_FORCE_EXACT):
        ix.set_tiers(flags)
        assert same(ix.search_batch_arrays(q, 10), before[10]), flags
    ix.set_tiers(0)
    assert ix.compact() == 0 and ix.store_stats()[4] == 1           # nothing dead: no second compaction is counted


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_small_index_direct_and_tiered(vdb, metric):
    rng = np.random.default_rng(7 + metric)
    m = Model(vdb, metric, rng.standard_normal((5000, 64)).astype(np.float32))
    churn(m, rng, 0.30, 0.10)
    q = rng.standard_normal((8, 64)).astype(np.float32)
    before = m.ix.search_batch_arrays(q, 10)
    assert m.compact() == 2000 and m.ix.store_stats()[0] == m.ix.len() == 3500
    for flags in (0, m.ix.TIERS_NO_DIRECT):
        m.ix.set_tiers(flags)
        assert same(m.check(q, 10), before), flags
        assert same(m.check(q[:1], 3), (before[0][:1, :3], before[1][:1, :3], np.minimum(before[2][:1], 3)))


# ------------------------------------------------------------------ 2. per-row state is moved, not recomputed
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_per_row_state_is_moved_bit_for_bit(vdb, metric):
    rng = np.random.default_rng(20 + metric)
    m = Model(vdb, metric, (rng.standard_normal((20_000, 48)) * rng.uniform(0.01, 30.0, (20_000, 1))).astype(np.float32))
    churn(m, rng, 0.25, 0.10)
    m.ix.debug_set_compact_bounce(512)                               # many chunks, bounced and direct
    info = m.ix.debug_row_info()
    assert info.shape[0] == 22_000
    if metric != 1:
        assert np.any(info[:, 3] != 0)                               # the margin column exists under Euclidean / Dot
    alive, ids_before = m.alive.copy(), m.ids.copy()
    m.compact()
    st = m.ix.store_stats()
    assert st[8] > 0 and st[9] > 0, st
    after = m.ix.debug_row_info()
    assert np.array_equal(after.view(np.uint32), info[alive].view(np.uint32))
    rows, ids = m.survivors()
    for i, id in enumerate(ids):
        assert m.ix.get_vector(int(id)).data.tobytes() == rows[i].tobytes(), id
    for id in np.setdiff1d(ids_before, ids):
        assert m.ix.get_vector(int(id)) is None


# ------------------------------------------------------------------ 3. edge shapes of the mover
def edge_dead(name, n, chunk):
    dead = np.zeros(n, dtype=bool)
    if name == "row0":
        dead[0] = True
    elif name == "last":
        dead[-1] = True
    elif name == "all_but_last":
        dead[:-1] = True
    elif name == "alternating":
        dead[::2] = True
    elif name == "block":                                            # one dead block longer than a chunk, live rows behind it
        dead[n // 5:n // 5 + chunk + chunk // 2 + 3] = True
    elif name == "late":                                             # dead rows only after the first chunk: the prefix stays
        dead[chunk + 37::3] = True
    return dead


@pytest.mark.parametrize("bounce", [0, 256])
@pytest.mark.parametrize("pattern", ["none", "row0", "last", "all_but_last", "alternating", "block", "late"])
@pytest.mark.parametrize("n,d", [(70001, 33), (3000, 7)])
def test_edge_shapes_of_the_mover(vdb, n, d, pattern, bounce):
    rng = np.random.default_rng(n + len(pattern))
    m = Model(vdb, 0, rng.standard_normal((n, d)).astype(np.float32))
    ix = m.ix
    ix.debug_set_compact_bounce(bounce)
    dead = edge_dead(pattern, n, 256)
    m.remove(np.nonzero(dead)[0])
    ld = (d + 31) // 32 * 32
    plan = ix.debug_compact_plan(pack(~dead), n, bounce_rows=bounce, ld=ld)
    q = rng.standard_normal((40, d)).astype(np.float32)
    before = ix.search_batch_arrays(q, 10)
    assert m.compact() == int(dead.sum())
    st = ix.store_stats()
    assert st[0] == st[1] == ix.len() == n - int(dead.sum())
    assert st[4] == (0 if pattern == "none" else 1)
    if pattern != "none":
        assert (st[8], st[9]) == (int((plan[:, 3] == 0).sum()), int((plan[:, 3] == 1).sum())), (st, plan[:6])
    if pattern == "all_but_last" or (pattern == "block" and bounce):
        assert st[8] > 0                                             # a gap wider than the chunk: moved directly
    if pattern in ("row0", "alternating"):
        assert st[9] > 0                                             # a gap narrower than the chunk: through the bounce buffer
    if pattern == "alternating" and bounce:
        assert st[8] > 0 and st[9] > 0
    if pattern == "late":
        assert plan[0][0] == (256 + 37) // 32 * 32                   # the rows below the first dead one are not touched
    assert same(m.check(q, 10, qsel=range(0, 40, 5)), before)
    assert same(m.check(q[:3], 4), (before[0][:3, :4], before[1][:3, :4], np.minimum(before[2][:3], 4)))
    rows, ids = m.survivors()
    step = 1 if (n < 10_000 or bounce) else 5                        # every id; at the large shape with one chunk, every fifth
    for i in range(0, ids.size, step):
        assert ix.get_vector(int(ids[i])).data.tobytes() == rows[i].tobytes(), ids[i]
    for id in np.nonzero(dead)[0][:2000]:
        assert ix.get_vector(int(id)) is None


# ------------------------------------------------------------------ 4. opt-in paths
def test_shadow_sample_cache_mask_and_large_k(vdb):
    rng = np.random.default_rng(4)
    n, d, nq = 90_000, 64, 48
    m = Model(vdb, 2, rng.standard_normal((n, d)).astype(np.float32))
    ix = m.ix
    ix.set_shadow(True)
    churn(m, rng, 0.15, 0.05)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    before = ix.search_batch_arrays(q, 10)
    assert ix.last_stats()["shadow_rows"] == 1
    assert m.compact() == int(n * 0.15) + int(n * 0.05)
    assert same(m.check(q, 10, qsel=range(0, nq, 4)), before) and ix.last_stats()["shadow_rows"] == 1
    for on in (False, True):
        ix.set_sample_cache(on)
        assert same(ix.search_batch_arrays(q, 10), before), on
    # a second round with the shadow in place: rows appended into the freed tail are converted, then everything moves again
    churn(m, rng, 0.10, 0.05)
    before = ix.search_batch_arrays(q, 10)
    m.compact()
    assert same(m.check(q, 10, qsel=range(0, nq, 6)), before) and ix.last_stats()["shadow_rows"] == 1
    ix.set_shadow(False)
    assert same(ix.search_batch_arrays(q, 10), before)
    # masked search: every third id eligible
    rows, ids = m.survivors()
    bits = int(ids.max()) + 1
    ok = np.zeros((bits + 63) // 64 * 64, dtype=np.uint8)
    ok[::3] = 1
    mask = np.packbits(ok, bitorder="little").view(np.uint64)
    gi, gd, gc = ix.search_batch_arrays(q[:16], 10, id_mask=mask, mask_bits=bits)
    elig = ok[ids.astype(np.int64)].astype(bool)
    for b in range(0, 16, 3):
        oi, od = oracle.flat_search(2, np.ascontiguousarray(rows[elig]), q[b], 10, ids=np.ascontiguousarray(ids[elig]))
        assert gc[b] == 10 and np.array_equal(gi[b], oi) and np.array_equal(gd[b].view(np.uint32), od.view(np.uint32)), b
    # large k, on whatever tier serves it at this size
    m.check(q[:8], 300, qsel=[0, 5])


# ------------------------------------------------------------------ 5. life goes on
def test_life_goes_on_after_a_compaction(vdb):
    rng = np.random.default_rng(5)
    n, d = 30_000, 40
    m = Model(vdb, 1, rng.standard_normal((n, d)).astype(np.float32))
    ix = m.ix
    q = rng.standard_normal((20, d)).astype(np.float32)
    churn(m, rng, 0.4, 0.1)
    ix.flush()
    cap = ix.store_stats()[2]
    assert m.compact() == int(n * 0.5) and ix.store_stats()[2] == cap    # shrink=False keeps the capacity
    assert m.compact() == 0                                              # twice in a row: nothing to take back
    m.check(q, 10, qsel=range(0, 20, 4))
    # adds (single and bulk) reuse the freed tail, removes and overwrites go on
    for i in range(50):
        m.add(10**6 + i, rng.standard_normal(d).astype(np.float32))
    m.add_bulk(rng.standard_normal((7000, d)).astype(np.float32), np.arange(2 * 10**6, 2 * 10**6 + 7000))
    assert ix.store_stats()[2] == cap
    m.remove(m.ids[m.alive][::5])
    m.add(int(m.ids[m.alive][3]), rng.standard_normal(d).astype(np.float32))         # overwrite
    m.check(q, 10, qsel=range(0, 20, 3))
    # compact with staged, not yet uploaded rows (they are uploaded first, then everything is compacted)
    for i in range(33):
        m.add(3 * 10**6 + i, rng.standard_normal(d).astype(np.float32))
    dead = int((~m.alive).sum())
    assert m.compact() == dead and ix.store_stats()[0] == ix.len() == int(m.alive.sum())
    assert ix.store_stats()[4] == 2 and ix.store_stats()[5] == int(n * 0.5) + dead
    m.check(q, 10, qsel=range(0, 20, 3))
    # rows of another dimension survive a compaction untouched
    ix.add(9 * 10**6, vdb.Vector(np.ones(3, dtype=np.float32)))
    m.remove(m.ids[m.alive][:100])
    m.compact()
    assert ix.get_vector(9 * 10**6).data.tobytes() == np.ones(3, dtype=np.float32).tobytes() and ix.len() == int(m.alive.sum()) + 1
    with pytest.raises(vdb.DimensionMismatch):
        ix.search_batch_arrays(q, 5)
    ix.remove(9 * 10**6)
    m.check(q, 10, qsel=[0, 7])
    # shrink: the capacity a fresh index of that many rows gets, and the store still grows from there
    m.remove(m.ids[m.alive][2000:])
    dead = int((~m.alive).sum())
    assert m.compact(shrink=True) == dead
    assert ix.store_stats()[2] == 2048 and ix.store_stats()[0] == 2000
    m.check(q, 10, qsel=[1, 8])
    m.add_bulk(rng.standard_normal((5000, d)).astype(np.float32), np.arange(4 * 10**6, 4 * 10**6 + 5000))
    m.check(q, 10, qsel=[2, 9])
    assert ix.compact(shrink=True) == 0 and ix.store_stats()[2] == 7168   # no dead row: only the re-allocation
    m.check(q, 10, qsel=[3])
    # removing every row still resets the index
    m.remove(m.ids[m.alive])
    assert ix.len() == 0 and ix.store_stats()[:3] == [0, 0, 0] and ix.compact() == 0
    assert ix.search_batch_arrays(q, 5)[2].sum() == 0
    ix.add_bulk(rng.standard_normal((100, 9)).astype(np.float32))        # another dimension is fine after the reset
    assert ix.len() == 100 and ix.dim() == 9


# ------------------------------------------------------------------ 6. refused while in flight
def test_refused_while_a_ticket_is_outstanding(vdb):
    import torch
    rng = np.random.default_rng(6)
    n, d, B, k = 80_000, 64, 64, 10
    m = Model(vdb, 0, rng.standard_normal((n, d)).astype(np.float32))
    m.remove(np.arange(0, n, 10))
    ix = m.ix
    ix.flush()
    dev = torch.device("cuda", 0)
    qh = rng.standard_normal((B, d)).astype(np.float32)
    q = torch.from_numpy(qh).to(dev)
    out = (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev))
    t = ix.search_batch_device_submit(q.data_ptr(), B, d, k, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    with pytest.raises(vdb.VectorDbError) as e_rm:
        ix.remove(1)
    with pytest.raises(vdb.VectorDbError) as e_c:
        ix.compact()
    assert str(e_c.value) == str(e_rm.value) and "in flight" in str(e_c.value)
    ix.search_batch_device_wait(t)
    torch.cuda.synchronize()
    got = (out[0].cpu().numpy().astype(np.uint64), out[1].cpu().numpy(), out[2].cpu().numpy().astype(np.uintp))
    m.check(qh, k, qsel=range(0, B, 8), got=got)
    assert m.compact() == n // 10 and ix.store_stats()[0] == ix.len()
    assert same(ix.search_batch_arrays(qh, k), got)


# ------------------------------------------------------------------ 7. auto-compaction
def test_auto_compaction_is_opt_in(vdb):
    rng = np.random.default_rng(70)
    n, d = 40_000, 32
    q = rng.standard_normal((16, d)).astype(np.float32)
    m = Model(vdb, 0, rng.standard_normal((n, d)).astype(np.float32))
    m.remove(np.arange(0, n, 2))
    m.check(q, 10, qsel=[0, 9])
    assert m.ix.store_stats()[:2] == [n, n // 2] and m.ix.store_stats()[4] == 0      # default: nothing changes for any caller
    with pytest.raises(vdb.VectorDbError):
        m.ix.set_auto_compact(1.5)
    m.ix.set_auto_compact(0.75)
    m.check(q, 10, qsel=[1])
    assert m.ix.store_stats()[0] == n                                                # 50 % dead is under the 75 % bar
    m.ix.set_auto_compact(0.25)
    got = m.check(q, 10, qsel=[0, 9])                                                # the search after the removes compacts first
    assert m.ix.store_stats()[0] == m.ix.len() == n // 2 and m.ix.store_stats()[4] == 1
    m.compact()                                                                      # (brings the model in step; nothing is dead)
    assert m.ix.store_stats()[4] == 1
    m.remove(m.ids[:n // 10])                                                        # 20 % dead: stays
    assert same(m.check(q, 10, qsel=[2]), m.fresh().search_batch_arrays(q, 10))
    assert m.ix.store_stats()[0] == n // 2 and got[2].min() == 10


# ------------------------------------------------------------------ 8. sharded handle
def test_sharded_handle(vdb):
    rng = np.random.default_rng(8)
    n, d = 60_000, 48
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((24, d)).astype(np.float32)
    sh = Model(vdb, 1, rows, devices=[0, 0, 0])
    sh.ix.set_exchange(sh.ix.EXCHANGE_PEER)
    plain = Model(vdb, 1, rows)
    for m in (sh, plain):
        churn(m, np.random.default_rng(81), 0.3, 0.1)
    lens = [sh.ix.shard_len(g) for g in range(3)]
    assert sum(lens) == sh.ix.len() == 42_000
    before = sh.ix.search_batch_arrays(q, 10)
    st0 = sh.ix.store_stats()
    assert st0[0] == n + 6000 and st0[1] == 42_000
    assert sh.compact() == 24_000 and plain.compact() == 24_000
    st = sh.ix.store_stats()
    assert st[0] == st[1] == sh.ix.len() == 42_000 and st[4] == 3 and st[5] == 24_000 and st[2] == st0[2]
    assert [sh.ix.shard_len(g) for g in range(3)] == lens            # rows do not change shards
    after = sh.check(q, 10, qsel=range(0, 24, 3))
    assert same(after, before) and same(after, plain.ix.search_batch_arrays(q, 10))
    sh.ix.set_auto_compact(0.2)
    sh.remove(sh.ids[::3])
    sh.check(q, 10, qsel=[0, 11])
    assert sh.ix.store_stats()[0] == sh.ix.len()


# ------------------------------------------------------------------ 9. store level
def test_vector_store_upserts(vdb):
    rng = np.random.default_rng(9)
    V, d = vdb.Vector, 24
    store = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    for rnd in range(5):
        for i in range(2000):
            store.insert_with_metadata(f"doc{i}", V(rng.standard_normal(d).astype(np.float32)),
                                       vdb.Metadata({"round": str(rnd), "parity": str((i + rnd) % 2)}))
    ix = store.index()
    assert ix.store_stats()[0] == 10_000 and store.len() == 2000
    qs = [(V(rng.standard_normal(d).astype(np.float32)), 10) for _ in range(6)]
    flt = vdb.MetadataFilter.Eq("parity", "1")
    before = (store.search(qs[0][0], 10), store.search_with_filter(qs[1][0], 10, flt), store.search_batch_prefiltered(qs, flt),
              store.search_batch(qs))
    assert store.compact() == 8000
    assert ix.store_stats()[0] == 2000 and store.len() == 2000
    after = (store.search(qs[0][0], 10), store.search_with_filter(qs[1][0], 10, flt), store.search_batch_prefiltered(qs, flt),
             store.search_batch(qs))
    assert after == before and len(before[0]) == 10 and all(len(r) == 10 for r in before[2])
    assert store.get("doc7") is not None and store.get_metadata("doc7").get("round") == "4"
    auto = vdb.VectorStore(vdb.DistanceMetric.Cosine, auto_compact=0.5)
    for rnd in range(4):
        for i in range(300):
            auto.insert(f"d{i}", V(rng.standard_normal(d).astype(np.float32)))
    assert auto.index().store_stats()[0] == 1200
    assert len(auto.search(qs[0][0], 5)) == 5 and auto.index().store_stats()[0] == 300

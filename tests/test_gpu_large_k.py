"""The screening tier's large-k range (112 < k <= 1024, rerank_large_kernel) and the shard merge above 2048 keys per query
(merge_rank_kernel).  Every answer is compared bit for bit: with the same search routed as before the range existed
(vdb_flat_set_large_k(h, 0)), with the exact scan (VDB_TIERS_FORCE_EXACT), and with the CPU oracle."""
import ctypes

import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu

TIMING = ("fused_kernel_ns", "host_enqueued_ns", "host_flags_ns", "host_total_ns")


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def same(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def counters(st):
    return {key: v for key, v in st.items() if key not in TIMING}


def check_oracle(metric, rows, q, k, res, qsel, ids=None, live=None):
    gi, gd, gc = res
    for b in qsel:
        kb = k[b] if not np.isscalar(k) else k
        oi, od = oracle.flat_search(metric, rows, q[b], kb, ids=ids, live=live)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi), b
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), b


def make(vdb, metric, rows, ids=None, devices=None):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, devices=devices)
    ix.add_bulk(rows, ids=ids)
    return ix


def exact(ix, q, k, **kw):
    ix.set_tiers(ix.TIERS_FORCE_EXACT)
    try:
        return ix.search_batch_arrays(q, k, **kw)
    finally:
        ix.set_tiers(0)


def test_large_k_at_1m_x_768_is_screened_and_exact(vdb):
    rng = np.random.default_rng(300)
    rows = rng.random((1_000_000, 768), dtype=np.float32) - 0.5
    q = rng.random((256, 768), dtype=np.float32) - 0.5
    ix = make(vdb, 1, rows)
    a = ix.search_batch_arrays(q, 300)
    st = ix.last_stats()
    assert st["bf16_screen"] == 1 and st["exact_queries"] == 0 and st["kprime"] >= 300, st
    ix.set_large_k(False)
    b = ix.search_batch_arrays(q, 300)
    assert ix.last_stats()["bf16_screen"] == 0
    ix.set_large_k(True)
    assert same(a, b)
    check_oracle(1, rows, q, 300, a, [0, 255])


def _rows(kind, rng, n, d):
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32)
    if kind == "gauss":
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "clustered":
        centres = rng.standard_normal((64, d)).astype(np.float32) * 4
        lab = np.sort(rng.integers(0, 64, n))                       # rows stored cluster by cluster
        return (centres[lab] + rng.standard_normal((n, d)).astype(np.float32) * 0.3).astype(np.float32)
    base = rng.random((n // 50, d), dtype=np.float32)                # every row 50 times: exact ties at every rank
    return np.ascontiguousarray(np.tile(base, (50, 1)))


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("kind", ["uniform", "gauss", "clustered", "ties"])
def test_large_k_sweep_matches_the_exact_scan(vdb, metric, kind):
    rng = np.random.default_rng(1000 + 10 * metric + len(kind))
    n, d, B = 300_000, 96, 12
    rows = _rows(kind, rng, n, d)
    q = rows[rng.integers(0, n, B)] + rng.standard_normal((B, d)).astype(np.float32) * 0.05
    q = np.ascontiguousarray(q, dtype=np.float32)
    ix = make(vdb, metric, rows)
    for k in (113, 200, 384, 1000, 1024, 1025):
        a = ix.search_batch_arrays(q, k)
        st = ix.last_stats()
        assert st["bf16_screen"] == (1 if k <= 1024 else 0), (k, st)
        assert same(a, exact(ix, q, k)), k
    a = ix.search_batch_arrays(q, 1000)
    check_oracle(metric, rows, q, 1000, a, [0, B - 1])
    ix.search_batch_arrays(q, 112)
    assert ix.last_stats()["kprime"] == 512                         # the small-k range is untouched


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_large_k_tombstones_sparse_ids_mask_and_ragged_ks(vdb, metric):
    rng = np.random.default_rng(77 + metric)
    n, d, B = 300_000, 64, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ids = rng.permutation(np.arange(n, dtype=np.uint64) * 7 + 3)    # sparse, not monotone
    ix = make(vdb, metric, rows, ids=ids)
    dead = rng.choice(n, 20_000, replace=False)
    for r in dead:
        ix.remove(int(ids[r]))
    live = np.ones(n, dtype=np.uint8)
    live[dead] = 0
    q = rng.standard_normal((B, d)).astype(np.float32)
    ks = np.array([10, 500] * (B // 2), dtype=np.uintp)
    a = ix.search_batch_arrays(q, ks)
    assert ix.last_stats()["bf16_screen"] == 1
    assert same(a, exact(ix, q, ks))
    check_oracle(metric, rows, q, ks, a, [0, 1], ids=ids, live=live)
    # an id mask: every id whose bit is set (ids below 2^21 here), ANDed with the tombstones
    mask_bits = 1 << 21
    mask = rng.integers(0, 2**63, mask_bits // 64, dtype=np.uint64) | rng.integers(0, 2**63, mask_bits // 64, dtype=np.uint64)
    a = ix.search_batch_arrays(q, 300, id_mask=mask, mask_bits=mask_bits)
    assert same(a, exact(ix, q, 300, id_mask=mask, mask_bits=mask_bits))
    bit = np.array([(i < mask_bits) and bool((int(mask[i // 64]) >> (i % 64)) & 1) for i in ids.tolist()], dtype=np.uint8)
    check_oracle(metric, rows, q, 300, a, [3], ids=ids, live=live & bit)


def test_large_k_boundaries(vdb):
    L = vdb._ffi.lib()
    k = 200
    m = L.vdb_flat_large_k_min_rows(k)
    assert m > 70_000 and L.vdb_flat_large_k_min_rows(112) == 0 and L.vdb_flat_large_k_min_rows(1025) == 0
    rng = np.random.default_rng(5)
    rows = rng.random((m, 32), dtype=np.float32)
    q = rng.random((8, 32), dtype=np.float32)
    ix = make(vdb, 0, rows)
    a = ix.search_batch_arrays(q, k)
    assert ix.last_stats()["bf16_screen"] == 1
    check_oracle(0, rows, q, k, a, [0, 7])
    ix2 = make(vdb, 0, rows[:m - 1])
    b = ix2.search_batch_arrays(q, k)
    assert ix2.last_stats()["bf16_screen"] == 0
    check_oracle(0, rows[:m - 1], q, k, b, [0, 7])
    # B = 1024 at k = 300 (wide passes) and the single-query entry point at k = 500
    rows = rng.standard_normal((300_000, 64)).astype(np.float32)
    q = rng.standard_normal((1024, 64)).astype(np.float32)
    ix = make(vdb, 2, rows)
    a = ix.search_batch_arrays(q, 300)
    assert ix.last_stats()["bf16_screen"] == 1
    assert same(a, exact(ix, q, 300))
    oi = np.zeros(500, dtype=np.uint64)
    od = np.zeros(500, dtype=np.float32)
    cnt = ctypes.c_size_t()
    rc = ix._L.vdb_flat_search(ix._h, q[5].ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 64, 500,
                               oi.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                               od.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(cnt))
    assert rc == 0 and ix.last_stats()["bf16_screen"] == 1
    ei, ed = oracle.flat_search(2, rows, q[5], 500)
    assert cnt.value == 500 and np.array_equal(oi, ei) and np.array_equal(od.view(np.uint32), ed.view(np.uint32))


def _outcome(fn):
    try:
        fn()
        return None
    except Exception as e:                                          # noqa: BLE001 -- the error class is what is compared
        return type(e).__name__


def test_large_k_errors_match_small_k(vdb):
    rng = np.random.default_rng(9)
    rows = rng.random((300_000, 32), dtype=np.float32)
    q = rng.random((4, 32), dtype=np.float32)
    z = rows.copy()
    z[1234] = 0.0
    nanr = rows.copy()
    nanr[777] = np.nan
    for metric, data, qq, want in ((1, z, q, "InvalidVector"), (0, nanr, q, None), (2, nanr, q, None),
                                   (0, rows, q[:, :16], "DimensionMismatch")):
        ix = make(vdb, metric, data)
        small = _outcome(lambda: ix.search_batch_arrays(qq, 10))
        large = _outcome(lambda: ix.search_batch_arrays(qq, 300))
        assert small == large, (metric, small, large)
        if want:
            assert large == want


def test_large_k_shadow_and_sample_cache_change_nothing(vdb):
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((300_000, 128)).astype(np.float32)
    q = rng.standard_normal((64, 128)).astype(np.float32)
    for metric in (0, 1):
        ix = make(vdb, metric, rows)
        a = ix.search_batch_arrays(q, 300)
        sa = counters(ix.last_stats())
        ix.set_shadow(True)
        b = ix.search_batch_arrays(q, 300)
        sb = counters(ix.last_stats())
        assert sb.pop("shadow_rows") == 1 and sa.pop("shadow_rows") == 0
        ix.set_sample_cache(False)
        c = ix.search_batch_arrays(q, 300)
        sc = counters(ix.last_stats())
        sc.pop("shadow_rows")
        assert sa["bf16_screen"] == 1 and sa == sb == sc, (sa, sb, sc)
        assert same(a, b) and same(a, c)


def test_sharded_handle_serves_large_k(vdb):
    rng = np.random.default_rng(12)
    n, d, B = 1_000_000, 64, 64
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    plain = make(vdb, 0, rows)
    sh = make(vdb, 0, rows, devices=[0] * 8)
    assert same(sh.search_batch_arrays(q, 300), plain.search_batch_arrays(q, 300))
    ks = np.array([10, 400, 300, 7] * (B // 4), dtype=np.uintp)       # max(ks) x 8 shards = 3200 keys per query
    assert same(sh.search_batch_arrays(q, ks), plain.search_batch_arrays(q, ks))
    del sh
    sh4 = make(vdb, 0, rows, devices=[0] * 4)
    a = sh4.search_batch_arrays(q[:16], 1000)
    assert same(a, plain.search_batch_arrays(q[:16], 1000))
    check_oracle(0, rows, q, 1000, a, [3])


@pytest.mark.parametrize("nparts,k", [(8, 300), (8, 1024)])
def test_merge_abi_above_2048_keys(vdb, nparts, k):
    import torch
    import sharded_mirror
    from vectordb_from_scratch_amd.sharded import merge_topk_hip
    g = torch.Generator().manual_seed(nparts * k)
    B = 5
    d = torch.randint(0, 40, (nparts, B, k), generator=g).to(torch.float32) * 0.25      # many cross-part distance ties
    ids = torch.randperm(nparts * B * k * 2, generator=g)[:nparts * B * k].view(nparts, B, k).to(torch.int64)
    ids[1, :, :] = ids[0, :, :]                                                          # equal (distance, id) pairs across parts
    d[1] = d[0]
    counts = torch.randint(k // 2, k + 1, (nparts, B), generator=g).to(torch.int32)
    counts[2, 0] = 0
    counts[3, 1] = k
    # every part ascending by (distance, id) over its first counts entries, as a search output is
    for p in range(nparts):
        for b in range(B):
            key = d[p, b].double() * 2**40 + ids[p, b].double()
            o = torch.argsort(key)
            d[p, b], ids[p, b] = d[p, b][o], ids[p, b][o]
    ids[1], d[1] = ids[0], d[0]
    ri, rd, rc = sharded_mirror.merge_topk_torch(ids, d, counts, k)
    dev = torch.device("cuda", 0)
    gi, gd, gc = merge_topk_hip(ids.to(dev), d.to(dev), counts.to(dev), k)
    torch.cuda.synchronize()
    gi, gd, gc = gi.cpu(), gd.cpu(), gc.cpu()
    assert torch.equal(gc, rc)
    for b in range(B):
        c = int(rc[b])
        assert torch.equal(gi[b, :c], ri[b, :c]) and torch.equal(gd[b, :c], rd[b, :c]), b
    # the packed all-gather layout: ids int64[B*k] | dists f32[B*k] | counts i32[B] | status i32 | pad
    nk = B * k
    words = B * (3 * k + 1) + 1
    words += words & 1
    packed = torch.zeros((nparts, words), dtype=torch.int32)
    for p in range(nparts):
        packed[p, :2 * nk] = ids[p].reshape(-1).view(torch.int32)
        packed[p, 2 * nk:3 * nk] = d[p].reshape(-1).view(torch.int32)
        packed[p, 3 * nk:3 * nk + B] = counts[p]
        packed[p, 3 * nk + B] = 3 * p
    packed = packed.to(dev)
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oc = torch.empty((B,), dtype=torch.int32, device=dev)
    os_ = torch.zeros((1,), dtype=torch.int32, device=dev)
    L = vdb._ffi.lib()
    rc2 = L.vdb_merge_topk_packed_device(0, ctypes.c_void_p(packed.data_ptr()), nparts, words, B, k,
                                         ctypes.c_void_p(oi.data_ptr()), ctypes.c_void_p(od.data_ptr()),
                                         ctypes.c_void_p(oc.data_ptr()), ctypes.c_void_p(os_.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc2 == 0
    assert int(os_.item()) == 3 * (nparts - 1)
    assert torch.equal(oc.cpu(), rc)
    for b in range(B):
        c = int(rc[b])
        assert torch.equal(oi.cpu()[b, :c], ri[b, :c]) and torch.equal(od.cpu()[b, :c], rd[b, :c]), b


def test_one_rank_shard_group_answers_k_2100(vdb):
    import torch
    from vectordb_from_scratch_amd.sharded import ShardGroup, group_search
    rng = np.random.default_rng(13)
    rows = rng.standard_normal((90_000, 48)).astype(np.float32)
    q = rng.standard_normal((6, 48)).astype(np.float32)
    grp = ShardGroup(ShardGroup.unique_id(), 0, 1, device=0)
    ix = make(vdb, 0, rows)
    gi, gd, gc = (t.cpu().numpy() for t in group_search(grp, ix)(torch.from_numpy(q).to(torch.device("cuda", 0)), 2100))
    pi, pd, pc = ix.search_batch_arrays(q, 2100)
    assert np.array_equal(gi.astype(np.uint64), pi) and np.array_equal(gd.view(np.uint32), pd.view(np.uint32))
    assert np.all(gc == 2100)


def test_store_filtered_search_over_eight_shards(vdb):
    rng = np.random.default_rng(14)
    n, d = 200_000, 32
    rows = rng.standard_normal((n, d)).astype(np.float32)
    colour = [("red", "blue", "green")[i % 3] for i in range(n)]
    flt = vdb.MetadataFilter.Eq("colour", "red")
    q = rng.standard_normal((3, d)).astype(np.float32)
    stores = []
    for devices in (None, [0] * 8):
        ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False, devices=devices)
        ix.add_bulk(rows)
        st = vdb.VectorStore(index=ix)
        st.attach_bulk_metadata(n, {"colour": colour})
        stores.append(st)
    plain, sharded = stores
    one_p = plain.search_with_filter(vdb.Vector(q[0]), 100, flt)
    one_s = sharded.search_with_filter(vdb.Vector(q[0]), 100, flt)
    assert one_p == one_s
    batch = [(vdb.Vector(q[b]), 100) for b in range(3)]
    bp = plain.search_batch_with_filter(batch, flt)
    bs = sharded.search_batch_with_filter(batch, flt)
    assert bp == bs and bp[0] == one_p
    for b in range(3):
        oi, od = oracle.flat_search(0, rows, q[b], 300)
        want = [(str(int(i)), float(x)) for i, x in zip(oi, od) if int(i) % 3 == 0][:100]
        assert [(r.id, r.distance) for r in bs[b]] == want, b

"""One batch, a filter per query (vdb_flat_search_batch_grouped, csrc/kernels_grouped.hip).  One sentence defines
the call: the answer for query b is what search_batch_arrays returns for that query ALONE under mask group_of[b] (under no mask for
GROUP_NONE).  Every test compares the grouped call with exactly that, query by query and bit for bit, with the sparse-filter route
of the single searches off and on, and a subset of the queries with the CPU oracle."""
import numpy as np
import pytest

import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def make_index(vdb, metric, rows, ids=None, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(rows, ids=ids)
    return ix


def pack_masks(id_lists, bits):
    """u64 [n_masks, words]: mask g has the bits of id_lists[g] set (ids below `bits` only)"""
    m = np.zeros((len(id_lists), (bits + 63) // 64), dtype=np.uint64)
    for g, ids in enumerate(id_lists):
        ids = np.asarray(ids, dtype=np.uint64)
        ids = ids[ids < np.uint64(bits)]
        if ids.size:
            np.bitwise_or.at(m[g], (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return m


def singles(ix, q, ks, masks, bits, group_of, modes=(0, 1)):
    """the definition: each query alone under its mask, once per sparse-filter mode of the single search; the modes must agree"""
    per_mode = []
    for mode in modes:
        ix.set_sparse_filter(mode)
        res = []
        for b in range(q.shape[0]):
            g = int(group_of[b])
            kw = {} if g == NONE else {"id_mask": masks[g], "mask_bits": bits}
            i, d, c = ix.search_batch_arrays(q[b:b + 1], int(ks[b]), **kw)
            res.append((i[0, :c[0]].copy(), d[0, :c[0]].view(np.uint32).copy()))
        per_mode.append(res)
    ix.set_sparse_filter(0)
    for other in per_mode[1:]:
        for b, (x, y) in enumerate(zip(per_mode[0], other)):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), ("the single searches disagree", b)
    return per_mode[0]


def assert_same(got, ref, what=""):
    gi, gd, gc = got
    for b, (ri, rd) in enumerate(ref):
        assert gc[b] == len(ri), (what, b, int(gc[b]), len(ri))
        assert np.array_equal(gi[b, :gc[b]], ri), (what, b, gi[b, :gc[b]], ri)
        assert np.array_equal(gd[b, :gc[b]].view(np.uint32), rd), (what, b)


def assert_oracle(metric, rows, q, ks, got, qsel, eligible_of, ids=None):
    gi, gd, gc = got
    for b in qsel:
        oi, od = oracle.flat_search(metric, rows, q[b], int(ks[b]), ids=ids, live=eligible_of(b).astype(np.uint8))
        assert gc[b] == len(oi), (b, int(gc[b]), len(oi))
        assert np.array_equal(gi[b, :gc[b]], oi) and np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), b


# ------------------------------------------------------------------ 1. tile edges, every metric, every dimension class
# list lengths {0, 1, 63, 64, 65, 129}; query counts {1, 63, 64, 65} and two more; 300 queries = two passes; the groups shuffled
# through the batch; a mask nobody references with garbage beyond mask_bits; unfiltered queries mixed in; k above several E_g
LENS = [0, 1, 63, 64, 65, 129]
COUNTS = [1, 63, 64, 65, 40, 37]


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("d", [1, 31, 32, 33, 100])
def test_tile_edges_differential_and_oracle(vdb, metric, d):
    rng = np.random.default_rng(1000 * metric + d)
    n, k = 3000, 10
    rows = (rng.standard_normal((n, d)) + (0.5 if d == 1 else 0.0)).astype(np.float32)
    rows[rows == 0] = 1.0
    ix = make_index(vdb, metric, rows)
    perm_rows = rng.permutation(n)
    lists, at = [], 0
    for E in LENS:
        lists.append(np.sort(perm_rows[at:at + E]))
        at += E
    bits = n
    masks = pack_masks(lists + [np.arange(n)], bits)
    masks[6, -1] = ~np.uint64(0)                                   # the unreferenced mask: garbage at and beyond mask_bits (3000 = 46 * 64 + 56)
    group_of = np.concatenate([np.full(c, g, dtype=np.uint32) for g, c in enumerate(COUNTS)] + [np.full(30, NONE, dtype=np.uint32)])
    rng.shuffle(group_of)
    nq = group_of.size
    assert nq == 300 and 6 not in group_of
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[np.abs(q).sum(axis=1) == 0] = 1.0
    ks = rng.integers(1, k + 1, size=nq)
    ref = singles(ix, q, np.full(nq, k), masks, bits, group_of)
    got = ix.search_batch_grouped(q, k, group_of, id_masks=masks, mask_bits=bits)
    st = ix.grouped_stats()
    assert_same(got, ref, "scalar k")
    for g, E in enumerate(LENS):                                   # k > E_g: the count is E_g
        assert (got[2][group_of == g] == min(k, E)).all(), (g, E)
    assert (got[2][group_of == NONE] == k).all()
    n_scan = sum(c for c, E in zip(COUNTS, LENS) if E)
    assert st[0] == nq and st[1] == 6 and st[2] == n_scan and st[3] == 0 and st[4] == 30 and st[7] == 2, st
    assert st[5] == sum(LENS)
    # per-query ks: the prefix property
    got_ks = ix.search_batch_grouped(q, 0, group_of, id_masks=masks, mask_bits=bits, ks=ks)
    assert_same(got_ks, [(ri[:kb], rd[:kb]) for (ri, rd), kb in zip(ref, ks)], "per-query ks")

    def eligible_of(b):
        e = np.zeros(n, dtype=bool)
        if group_of[b] == NONE:
            e[:] = True
        else:
            e[lists[group_of[b]]] = True
        return e
    assert_oracle(metric, rows, q, np.full(nq, k), got, range(0, nq, 23), eligible_of)


# ------------------------------------------------------------------ 2. numbers of masks; a mask shared by non-adjacent queries
@pytest.mark.parametrize("n_masks", [1, 2, 7, 40])
def test_mask_counts(vdb, n_masks):
    rng = np.random.default_rng(n_masks)
    n, d, k, nq = 5000, 33, 5, 90
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 1, rows)
    tenant = rng.integers(0, n_masks, size=n)
    lists = [np.nonzero(tenant == g)[0] for g in range(n_masks)]
    masks = pack_masks(lists, n)
    group_of = (np.arange(nq) % n_masks).astype(np.uint32)         # mask g at queries g, g + n_masks, ...: never adjacent for n_masks > 1
    q = rng.standard_normal((nq, d)).astype(np.float32)
    ref = singles(ix, q, np.full(nq, k), masks, n, group_of)
    got = ix.search_batch_grouped(q, k, group_of, id_masks=masks, mask_bits=n)
    assert_same(got, ref)
    st = ix.grouped_stats()
    assert st[1] == n_masks and st[2] == nq and st[5] == n and st[7] == 1, st

    def eligible_of(b):
        return tenant == group_of[b]
    assert_oracle(1, rows, q, np.full(nq, k), got, [0, 41, 89], eligible_of)


# ------------------------------------------------------------------ 3. store states
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_store_states(vdb, metric):
    rng = np.random.default_rng(30 + metric)
    n, d, k = 4000, 31, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    # exact duplicates: rows 10, 11 in one group (A), row 12 = row 10 in another (B)
    rows[11] = rows[10]
    rows[12] = rows[10]
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(3)      # non-monotone ids: the id-rank path
    ids[20] = np.uint64(1 << 32) + np.uint64(5)                    # an id at or above 2^32: ineligible under every mask
    bits = int(np.sort(ids)[-40])                                  # ... and the ids at or above mask_bits too (the largest 40)
    ix = make_index(vdb, metric, rows, ids=ids)
    live = np.ones(n, dtype=bool)
    for r in range(5, n, 9):
        if r not in (10, 11, 12):
            ix.remove(int(ids[r]))
            live[r] = False
    grp = rng.integers(0, 3, size=n)
    grp[[10, 11]] = 0
    grp[12] = 1
    lists = [ids[grp == g] for g in range(3)]                      # tombstoned rows and out-of-range ids included: the mask admits them, the store does not
    masks = pack_masks(lists, bits)
    nq = 70
    group_of = rng.integers(0, 3, size=nq).astype(np.uint32)
    group_of[::11] = NONE
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[0] = rows[10]                                                # the duplicates tie at the smallest distance: the lower id first
    group_of[0], group_of[1] = 0, 1
    q[1] = rows[10]
    ref = singles(ix, q, np.full(nq, k), masks, bits, group_of)
    got = ix.search_batch_grouped(q, k, group_of, id_masks=masks, mask_bits=bits)
    assert_same(got, ref)
    lo, hi = sorted([int(ids[10]), int(ids[11])])
    if lo < bits and hi < bits:
        first_two = got[0][0, :2].tolist()
        assert first_two == [lo, hi] or metric == 2, first_two     # (Dot ranks by -q.x: the duplicates need not be nearest)
        assert got[1][0, 0].view(np.uint32) == got[1][0, 1].view(np.uint32) or metric == 2
    assert int(ids[20]) not in got[0][group_of != NONE].tolist()

    def eligible_of(b):
        if group_of[b] == NONE:
            return live
        return live & (grp == group_of[b]) & (ids < np.uint64(bits))
    assert_oracle(metric, rows, q, np.full(nq, k), got, [0, 1, 2, 11, 40, 69], eligible_of, ids=ids)


# ------------------------------------------------------------------ 4. capacity fallback
def test_capacity_fallback(vdb):
    rng = np.random.default_rng(4)
    n, d, k = 140000, 8, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 0, rows)
    big = np.arange(0, 135000)                                     # more than 131072 eligible rows
    small_a = rng.choice(n, size=500, replace=False)
    small_b = rng.choice(n, size=65, replace=False)
    masks = pack_masks([big, small_a, small_b], n)
    group_of = np.array([0, 1, 2, 0, NONE, 1, 0, 2], dtype=np.uint32)
    q = rng.standard_normal((group_of.size, d)).astype(np.float32)
    ref = singles(ix, q, np.full(8, k), masks, n, group_of, modes=(0,))
    got = ix.search_batch_grouped(q, k, group_of, id_masks=masks, mask_bits=n)
    assert_same(got, ref)
    st = ix.grouped_stats()
    assert st[:5] == [8, 3, 4, 3, 1] and st[5] == 565 and st[7] == 1, st
    # k beyond the select: every non-empty group takes the ordinary search
    sel = np.array([1, 2, 4])
    ref = singles(ix, q[sel], np.full(3, 2049), masks, n, group_of[sel], modes=(0,))
    got = ix.search_batch_grouped(q[sel], 2049, group_of[sel], id_masks=masks, mask_bits=n)
    assert_same(got, ref)
    assert got[2].tolist() == [500, 65, 2049]
    st = ix.grouped_stats()
    assert st[:5] == [3, 2, 0, 2, 1] and st[6] == 0, st


# ------------------------------------------------------------------ 5. errors, in their order
def test_errors_in_order(vdb):
    rng = np.random.default_rng(5)
    n, d, k = 3000, 32, 4
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((6, d)).astype(np.float32)
    masks = pack_masks([np.arange(0, 100), np.arange(100, 300)], n)
    go = np.array([0, 1, NONE, 0, 1, 1], dtype=np.uint32)
    E = vdb.IndexError_
    # 1. an empty index or k = 0: counts 0 before any check (a null group_of, a bad index)
    empty = vdb.GpuFlatIndex(vdb.DistanceMetric.Cosine, keep_host_copy=False)
    assert (empty.search_batch_grouped(q, k, None, id_masks=masks, mask_bits=n)[2] == 0).all()
    assert (empty.search_batch_grouped(q, k, np.full(6, 9), id_masks=masks, mask_bits=n)[2] == 0).all()
    c = make_index(vdb, 1, rows)
    assert (c.search_batch_grouped(q, 0, None, id_masks=masks, mask_bits=n)[2] == 0).all()
    # 2. argument errors
    with pytest.raises(E, match="group_of"):
        c.search_batch_grouped(q, k, None, id_masks=masks, mask_bits=n)
    with pytest.raises(E, match="names mask 2 of 2"):
        c.search_batch_grouped(q, k, np.array([0, 1, 2, 0, 1, 1]), id_masks=masks, mask_bits=n)
    with pytest.raises(E, match="at most 1024"):
        c.search_batch_grouped(q, k, go, id_masks=np.zeros((1025, masks.shape[1]), dtype=np.uint64), mask_bits=n)
    L, ct = vdb._ffi.lib(), __import__("ctypes")
    outs = (np.zeros((6, k), dtype=np.uint64), np.zeros((6, k), dtype=np.float32), np.zeros(6, dtype=np.uintp))
    ptrs = (outs[0].ctypes.data_as(ct.POINTER(ct.c_uint64)), outs[1].ctypes.data_as(ct.POINTER(ct.c_float)), outs[2].ctypes.data_as(ct.POINTER(ct.c_size_t)))
    qp, gp = q.ctypes.data_as(ct.POINTER(ct.c_float)), go.ctypes.data_as(ct.POINTER(ct.c_uint32))
    assert L.vdb_flat_search_batch_grouped(c._h, qp, 6, d, None, k, None, 2, n, gp, k, *ptrs) == vdb._ffi.ERR_INVALID_ARGUMENT
    assert "null mask array" in vdb._ffi.last_error()[0]
    assert L.vdb_flat_search_batch_grouped_filtered(c._h, qp, 6, d, None, k, None, 2, gp, k, *ptrs) == vdb._ffi.ERR_INVALID_ARGUMENT
    arr = (ct.c_void_p * 2)(None, None)
    assert L.vdb_flat_search_batch_grouped_filtered(c._h, qp, 6, d, None, k, arr, 2, gp, k, *ptrs) == vdb._ffi.ERR_INVALID_ARGUMENT
    assert "mask 0 is null" in vdb._ffi.last_error()[0]
    # ... and all of them before the dimension check
    with pytest.raises(E, match="group_of"):
        c.search_batch_grouped(q[:, :7], k, None, id_masks=masks, mask_bits=n)
    # 3. dimension mismatch
    with pytest.raises(vdb.DimensionMismatch):
        c.search_batch_grouped(q[:, :7], k, go, id_masks=masks, mask_bits=n)
    # 5. a zero-norm query anywhere in the batch (also in a group nothing is eligible for), before 6. any NaN
    c.add(n, vdb.Vector([float("nan")] + [1.0] * (d - 1)))         # id n: a NaN row, eligible for mask 2 only
    masks3 = pack_masks([np.arange(0, 100), np.arange(100, 300), [n], []], n + 1)
    qz = q.copy()
    qz[4] = 0.0
    with pytest.raises(vdb.InvalidVector):
        c.search_batch_grouped(qz, k, np.array([0, 1, 2, 0, 3, 1]), id_masks=masks3, mask_bits=n + 1)
    # 6. the NaN row fails the call only when a query references its group
    with pytest.raises(vdb.NanDistance):
        c.search_batch_grouped(q, k, np.array([0, 1, 2, 0, 3, 1]), id_masks=masks3, mask_bits=n + 1)
    go_ok = np.array([0, 1, 3, 0, 3, 1], dtype=np.uint32)
    got = c.search_batch_grouped(q, k, go_ok, id_masks=masks3, mask_bits=n + 1)
    assert got[2].tolist() == [k, k, 0, k, 0, k]
    assert_same(got, singles(c, q, np.full(6, k), masks3, n + 1, go_ok))
    # 4. under Cosine one live zero-norm row fails the call, masked or not
    c.add(n + 1, vdb.Vector([0.0] * d))
    with pytest.raises(vdb.InvalidVector):
        c.search_batch_grouped(q, k, go_ok, id_masks=masks3, mask_bits=n + 1)
    c.remove(n + 1)
    assert c.search_batch_grouped(q, k, go_ok, id_masks=masks3, mask_bits=n + 1)[2].tolist() == [k, k, 0, k, 0, k]


def test_outstanding_ticket_refuses_the_call(vdb):
    import torch
    rng = np.random.default_rng(6)
    n, d, k, B = 20000, 16, 4, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    masks = pack_masks([np.arange(0, 100)], n)
    go = np.zeros(B, dtype=np.uint32)
    ix = make_index(vdb, 0, rows)
    dev = torch.device("cuda", 0)
    qt = torch.from_numpy(q).to(dev)
    outs = (torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    t = ix.search_batch_device_submit(qt.data_ptr(), B, d, k, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
    try:
        with pytest.raises(vdb.IndexError_, match="in flight"):
            ix.search_batch_grouped(q, k, go, id_masks=masks, mask_bits=n)
    finally:
        ix.search_batch_device_wait(t)
    assert (ix.search_batch_grouped(q, k, go, id_masks=masks, mask_bits=n)[2] == k).all()


def test_sharded_handle_is_refused(vdb):
    rng = np.random.default_rng(9)
    n, d, k, B = 4000, 16, 4, 8
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((B, d)).astype(np.float32)
    masks = pack_masks([np.arange(0, 100)], n)
    go = np.zeros(B, dtype=np.uint32)
    sh = make_index(vdb, 0, rows, devices=[0, 0])
    with pytest.raises(vdb.IndexError_, match="sharded"):
        sh.search_batch_grouped(q, k, go, id_masks=masks, mask_bits=n)
    with pytest.raises(vdb.IndexError_, match="sharded"):
        sh.grouped_stats()


# ------------------------------------------------------------------ 6. compiled masks and the store
@pytest.mark.parametrize("device_filter", [False, True])
def test_store_search_batch_with_filters(vdb, device_filter):
    rng = np.random.default_rng(7)
    n, d, nq = 6000, 32, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 0, rows)
    st = vdb.VectorStore(index=ix)
    tenant = rng.choice(["a", "b", "c", "d"], size=n, p=[0.6, 0.3, 0.09, 0.01]).astype(object)
    tier = np.where(rng.random(n) < 0.5, "gold", None).astype(object)
    st.attach_bulk_metadata(n, {"tenant": tenant, "tier": tier})
    st.set_device_filter(device_filter)
    F = vdb.MetadataFilter
    make = [lambda: F.Eq("tenant", "a"), lambda: F.Eq("tenant", "d"), lambda: F.Ne("tenant", "a"),
            lambda: F.And([F.Eq("tenant", "b"), F.Eq("tier", "gold")]), lambda: F.Eq("tenant", "nobody"), lambda: None]
    which = rng.integers(0, len(make), size=nq)
    filters = [make[w]() for w in which]                           # equal filters are DIFFERENT objects
    queries = [(vdb.Vector(rng.standard_normal(d).astype(np.float32)), int(rng.integers(1, 12))) for _ in range(nq)]
    got = st.search_batch_with_filters(queries, filters)
    stats = ix.grouped_stats()
    assert stats[0] == nq and stats[1] == len({int(w) for w in which if w != 5}), stats   # equal filters collapse to one group
    assert stats[2] + stats[4] == nq - int((which == 4).sum())
    for b in range(nq):
        if filters[b] is None:
            want = st.search_batch([queries[b]])[0]
        else:
            want = st.search_batch_prefiltered([queries[b]], filters[b])[0]
        assert [(r.id, np.float32(r.distance).view(np.uint32)) for r in got[b]] == [(r.id, np.float32(r.distance).view(np.uint32)) for r in want], b
    assert all(len(got[b]) == 0 for b in range(nq) if which[b] == 4)
    with pytest.raises(ValueError):
        vdb.VectorStore(index=vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 20, 20), seed=1)).search_batch_with_filters(queries, filters)


def test_compiled_masks_of_different_lengths(vdb):
    rng = np.random.default_rng(8)
    n, d, k, nq = 3000, 100, 6, 20
    rows = rng.standard_normal((n, d)).astype(np.float32)
    ix = make_index(vdb, 2, rows)
    T = vdb.MetaTable
    table = T(0)
    codes = rng.integers(0, 3, size=n).astype(np.int32)
    table.set_codes(0, 0, codes)
    table.set_present(0, n, True)
    cms = [table.compile([(T.EQ, 0, 0)], n), table.compile([(T.EQ, 0, 1)], n - 1000), None, table.compile([(T.EQ, 0, 2)], 70)]
    try:
        go = rng.choice([0, 1, 3, NONE], size=nq).astype(np.uint32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        got = ix.search_batch_grouped(q, k, go, compiled_masks=cms)
        lists = [np.nonzero(codes == 0)[0], np.nonzero(codes[:n - 1000] == 1)[0], [], np.nonzero(codes[:70] == 2)[0]]
        masks = pack_masks(lists, n)
        assert_same(got, singles(ix, q, np.full(nq, k), masks, n, go))
        assert ix.grouped_stats()[1] == len(set(go.tolist()) - {NONE})
    finally:
        for cm in cms:
            if cm is not None:
                cm.release()
        table.close()


def test_compiled_mask_on_another_device(vdb):
    T = vdb.MetaTable
    try:
        t = T(1)
    except vdb.IndexError_ as e:
        assert "out of range" in str(e)
        pytest.skip("needs a second GPU to hold the table")
    rng = np.random.default_rng(10)
    n, d = 3000, 16
    ix = make_index(vdb, 0, rng.standard_normal((n, d)).astype(np.float32))
    t.set_present(0, n, True)
    cm = t.compile([(T.CONST, 0, 1)], n)
    try:
        q = rng.standard_normal((2, d)).astype(np.float32)
        with pytest.raises(vdb.IndexError_, match="lives on device 1"):
            ix.search_batch_grouped(q, 3, np.array([0, NONE]), compiled_masks=[cm])
        # ... but a mask nobody references is never looked at
        assert ix.search_batch_grouped(q, 3, np.array([NONE, NONE]), compiled_masks=[cm])[2].tolist() == [3, 3]
    finally:
        cm.release()
        t.close()

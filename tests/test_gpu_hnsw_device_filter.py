"""HNSW search under a filter compiled on the device (include/vdb_hnsw.h vdb_hnsw_search_batch_filtered):
hnsw_present_mask_kernel alone against numpy `mask & present`; the filtered call against the masked call under the same words
on every route (device walk, host traversal, filter scan), bit for bit; the early-out when nothing is eligible and the errors
that stay; a VectorStore over a GpuHnswIndex with set_device_filter on against off, also through the server; the refusals.

No graph of at most 1500 nodes can overflow the pre-filtered walk (its candidate heap holds 11264 entries, a node is pushed
once), and the one shape of tests/hnsw_limits.py that does (45000 x 48) takes far longer than a test here may: the mask's lazy
copy back to the host is covered through set_traversal(True), which runs the same code in front of the same traversal."""
import ctypes

import numpy as np
import pytest

import filter_programs as fp
from conftest import load_package
from hnsw_filter_restatement import Walker, eligible_fn
from test_gpu_device_filter import as_arrays, popcount, read_mask
from test_gpu_hnsw_filter import build_pair, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def table_of(vdb, elig):
    """a MetaTable whose column 0 holds elig as codes 0 / 1, every id present: EQ 1 compiles to elig, CONST 1 to all ones"""
    t = vdb.MetaTable(0)
    t.set_codes(0, 0, np.asarray(elig).astype(np.int32))
    t.set_present(0, len(elig), True)
    return t


def programs(T):
    return {"random": [(T.EQ, 0, 1)], "all ones": [(T.CONST, 0, 1)], "none": [(T.CONST, 0, 0)]}


def pack(bits_bool):
    out = np.zeros((bits_bool.size + 63) // 64 * 8, dtype=np.uint8)
    pb = np.packbits(bits_bool, bitorder="little")
    out[:pb.size] = pb
    return out.view(np.uint64)


def check_present_mask(g, table, prog, bits, present):
    """debug_present_mask == the compiled words & present over min(bits, node ids) bits, word for word, and its count"""
    with table.compile(prog, bits) as cm:
        src, _ = read_mask(cm)
        got, count = g.debug_present_mask(cm)
    nb = min(bits, present.size)
    want = np.unpackbits(src.view(np.uint8), bitorder="little")[:nb].astype(bool) & present[:nb]
    assert got.size == (nb + 63) // 64, (bits, got.size)
    assert np.array_equal(got, pack(want)), (bits, np.flatnonzero(got != pack(want))[:5])
    assert count == int(want.sum()) == popcount(got), (bits, count)
    return count


# ------------------------------------------------------------------ 1. the kernel alone
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 4097])
def test_present_mask_kernel_against_numpy(vdb, n):
    T, V = vdb.MetaTable, vdb.Vector
    rng = np.random.default_rng(n)
    d = 4
    rows = rng.standard_normal((n, d)).astype(np.float32)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 16, 16), seed=n)
    table = table_of(vdb, rng.random(n + 100) < 0.5)
    progs = programs(T)
    present = np.zeros(n - 1, dtype=bool)
    if n > 1:
        g.build_batch((np.arange(n - 1, dtype=np.uint64), rows[:n - 1]))
        present[:] = True
    assert check_present_mask(g, table, progs["all ones"], n + 100, present) == n - 1     # the mirror as the bulk build left it (n = 1: an empty graph)
    g.add(n - 1, V(rows[n - 1]))                                           # ONE add behind it: the mirror is brought up to date incrementally
    present = np.append(present, True)
    assert check_present_mask(g, table, progs["all ones"], n, present) == n
    gone = np.arange(0, n, 3)
    for i in gone:
        g.remove(int(i))
    present[gone] = False
    assert check_present_mask(g, table, progs["all ones"], n, present) == n - gone.size
    for i in gone[::2]:                                                    # ids inserted again are present again
        g.add(int(i), V(rng.standard_normal(d).astype(np.float32)))
    present[gone[::2]] = True
    for bits in sorted({1, max(n // 2, 1), n, n + 1, n + 100}):            # below, at and above the node count
        for name, prog in progs.items():
            count = check_present_mask(g, table, prog, bits, present)
            if name == "all ones":
                assert count == int(present[:bits].sum())
            if name == "none":
                assert count == 0
    table.close()


def test_present_mask_over_sparse_ids(vdb):
    """ids 50 .. 199 and 261 .. 299 were never inserted: row_of has holes below the mirror's id count"""
    T = vdb.MetaTable
    rng = np.random.default_rng(77)
    ids = np.concatenate([np.arange(50), np.arange(200, 261)]).astype(np.uint64)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 16, 16), seed=3)
    g.build_batch((ids, rng.standard_normal((ids.size, 4)).astype(np.float32)))
    g.search_batch_arrays(np.zeros((1, 4), np.float32), 1, 16)
    g.add(300, vdb.Vector(rng.standard_normal(4).astype(np.float32)))
    present = np.zeros(301, dtype=bool)
    present[ids.astype(np.int64)] = True
    present[300] = True
    table = table_of(vdb, rng.random(400) < 0.5)
    for bits in (1, 50, 51, 150, 200, 201, 300, 301, 400):
        for name, prog in programs(T).items():
            count = check_present_mask(g, table, prog, bits, present)
            if name == "all ones":
                assert count == int(present[:bits].sum())
    table.close()


# ------------------------------------------------------------------ 2. filtered == masked, on every route
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("n,d,m,efc,ef", [(300, 8, 4, 32, 32), (1500, 48, 16, 200, 200)])
def test_filtered_equals_masked_on_every_route(vdb, metric, n, d, m, efc, ef):
    T = vdb.MetaTable
    rng = np.random.default_rng(100 + n + metric)
    rows = rng.standard_normal((n, d)).astype(np.float32)             # Gaussian: no distance ties (the restatement uses heapq)
    qs = rng.standard_normal((8, d)).astype(np.float32)
    k = 10
    anchored = metric == 0 and n == 300                                # one case is also held against the restatement on the oracle's graph
    if anchored:
        g, o = build_pair(vdb, metric, rows, m, efc, seed=5)
        w = Walker(o, metric, {i: rows[i] for i in range(n)})
    else:
        g = vdb.GpuHnswIndex(vdb.DistanceMetric(metric), vdb.HnswParams.new(m, efc, 50), seed=5)
        g.build_batch((np.arange(n, dtype=np.uint64), rows))
    for sel in (0.5, 0.1, 0.01):
        elig = rng.random(n) < sel
        table = table_of(vdb, elig)
        with table.compile([(T.EQ, 0, 1)], n) as cm:
            words, eligible = read_mask(cm)
            bits = cm.bits
            assert bits == n and eligible == int(elig.sum())
            # the device walk
            before = g.stats()
            dev = g.search_batch_arrays(qs, k, ef, compiled_mask=cm)
            after = g.stats()
            if eligible:
                assert after["device_queries"] - before["device_queries"] + after["host_redone"] - before["host_redone"] == len(qs)
            masked = g.search_batch_arrays(qs, k, ef, id_mask=words, mask_bits=bits)
            again = g.stats()
            assert same(dev, masked), (sel, "device walk")
            assert [again[x] - after[x] for x in ("gpu_launches", "device_queries", "host_redone")] == \
                   [after[x] - before[x] for x in ("gpu_launches", "device_queries", "host_redone")], sel
            # the host traversal: the ANDed mask comes back from the device once
            g.set_traversal(True)
            host = g.search_batch_arrays(qs, k, ef, compiled_mask=cm)
            rounds = g.stats()["last_search_rounds"]
            host_masked = g.search_batch_arrays(qs, k, ef, id_mask=words, mask_bits=bits)
            g.set_traversal(False)
            assert same(host, host_masked) and same(host, dev), (sel, "host traversal")
            assert rounds == g.stats()["last_search_rounds"] and (rounds > 0) == (eligible > 0)
            # the filter scan, on both sides
            g.set_filter_scan(n)
            s0 = g.stats()
            scan = g.search_batch_arrays(qs, k, ef, compiled_mask=cm)
            s1 = g.stats()
            scan_masked = g.search_batch_arrays(qs, k, ef, id_mask=words, mask_bits=bits)
            g.set_filter_scan(0)
            assert same(scan, scan_masked), (sel, "filter scan")
            assert s1["gpu_launches"] - s0["gpu_launches"] == (1 if eligible else 0) and s1["device_queries"] == s0["device_queries"]
            assert np.all(scan[2] == min(k, eligible))
        table.close()
        if anchored and sel == 0.5:
            di, dd, dc = dev
            for b in range(len(qs)):
                wi, wd = w.search(qs[b], k, ef, eligible_fn(elig))
                assert dc[b] == wi.size and np.array_equal(di[b, :dc[b]], wi), (sel, b)
                assert np.array_equal(dd[b, :dc[b]].view(np.uint32), wd.view(np.uint32)), (sel, b)


def test_filtered_search_over_removed_and_readded_ids(vdb):
    """the compiled mask admits ids the graph has dropped (the store's table would not; a raw table may): never returned, and
    the three routes still equal the masked call"""
    T = vdb.MetaTable
    rng = np.random.default_rng(4)
    n, d, k, ef = 300, 8, 5, 40
    rows = rng.standard_normal((n, d)).astype(np.float32)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 32, 50), seed=2)
    g.build_batch((np.arange(n, dtype=np.uint64), rows))
    gone = np.arange(0, n, 3)
    for i in gone:
        g.remove(int(i))
    for i in gone[::4]:
        g.add(int(i), vdb.Vector(rng.standard_normal(d).astype(np.float32)))
    qs = rng.standard_normal((5, d)).astype(np.float32)
    only_gone = np.zeros(n, dtype=bool)
    only_gone[np.setdiff1d(gone, gone[::4])] = True
    for elig, nothing in ((only_gone, True), (rng.random(n) < 0.5, False)):
        table = table_of(vdb, elig)
        with table.compile([(T.EQ, 0, 1)], n + 100) as cm:              # bits beyond the last id name nothing
            words, _ = read_mask(cm)
            for scan in (0, n):
                g.set_filter_scan(scan)
                for host in (False, True):
                    g.set_traversal(host)
                    got = g.search_batch_arrays(qs, k, ef, compiled_mask=cm)
                    assert same(got, g.search_batch_arrays(qs, k, ef, id_mask=words, mask_bits=cm.bits)), (scan, host)
                    assert np.all(got[2] == 0) == nothing
                    assert all(elig[int(i)] and not only_gone[int(i)] for b in range(len(qs)) for i in got[0][b, :got[2][b]])
            g.set_traversal(False)
            g.set_filter_scan(0)
        table.close()


# ------------------------------------------------------------------ 4. nothing eligible
def test_nothing_eligible_walks_nothing_and_keeps_the_errors(vdb):
    T, V = vdb.MetaTable, vdb.Vector
    rng = np.random.default_rng(3)
    n, d = 400, 16
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 64, 50), seed=9)
    g.build_batch((np.arange(n, dtype=np.uint64), rng.standard_normal((n, d)).astype(np.float32)))
    qs = rng.standard_normal((6, d)).astype(np.float32)
    g.search_batch_arrays(qs, 10, 60)
    table = table_of(vdb, np.zeros(n + 200, dtype=bool))
    beyond = np.zeros(n + 200, dtype=bool)
    beyond[n:] = True
    table2 = table_of(vdb, beyond)                                     # only ids the graph never held
    for t, prog, bits in ((table, [(T.EQ, 0, 1)], n), (table, [(T.CONST, 0, 0)], n + 200), (table2, [(T.EQ, 0, 1)], n + 200),
                          (table, [(T.CONST, 0, 1)], 0)):
        with t.compile(prog, bits) as cm:
            for host in (False, True):
                g.set_traversal(host)
                before = g.stats()
                _, _, c = g.search_batch_arrays(qs, 10, 60, compiled_mask=cm)
                after = g.stats()
                assert np.all(c == 0)
                assert all(after[x] == before[x] for x in ("gpu_launches", "device_queries", "host_redone", "gpu_distances")), (before, after)
                assert after["last_search_rounds"] == 0
            g.set_traversal(False)
            with pytest.raises(vdb.DimensionMismatch):
                g.search_batch_arrays(np.ones((1, d + 1), np.float32), 1, 16, compiled_mask=cm)
    table.close()
    table2.close()
    ix = vdb.GpuHnswIndex(vdb.DistanceMetric.Cosine, vdb.HnswParams.new(4, 32, 16))
    ix.add(0, V([1.0, 0.0])); ix.add(1, V([0.0, 1.0]))
    t = table_of(vdb, np.array([False, True]))
    for prog in ([(T.EQ, 0, 1)], [(T.CONST, 0, 0)]):                   # the walk, and the empty mask that skips it
        with t.compile(prog, 2) as cm:
            with pytest.raises(vdb.InvalidVector):
                ix.search_batch_arrays(np.zeros((1, 2), np.float32), 1, 16, compiled_mask=cm)
            with pytest.raises(vdb.DimensionMismatch):
                ix.search_batch_arrays(np.ones((1, 3), np.float32), 1, 16, compiled_mask=cm)
    with t.compile([(T.EQ, 0, 1)], 2) as cm:
        i, _, c = ix.search_batch_arrays(np.array([[1.0, 0.1]], np.float32), 2, 16, compiled_mask=cm)
        assert c[0] == 1 and i[0, 0] == 1
    t.close()


# ------------------------------------------------------------------ 5. the store and the server
def store_filters(F):
    return {"eq": F.Eq("color", "red"), "ne": F.Ne("size", "m"), "exists": F.Exists("shape"),
            "tree": F.And([F.Ne("color", "red"), F.Or([F.Exists("size"), F.And([F.Eq("shape", "square"), F.Ne("color", "blue")])])]),
            "nobody": F.And([F.Eq("color", "red"), F.Eq("color", "blue")]),
            "over the limit": F.Or([F.Eq("shape", "round")] * 513)}      # 1025 ops: compiled in numpy


def test_store_on_an_hnsw_index_device_filter_on_equals_off(vdb):
    F, M, V = vdb.MetadataFilter, vdb.Metadata, vdb.Vector
    rng = np.random.default_rng(12)
    n, d, k = 1200, 24, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((6, d)).astype(np.float32)
    ix = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 64, 50), seed=1)
    ix.build_batch((np.arange(n, dtype=np.uint64), rows))
    st = vdb.VectorStore.with_index(ix)
    st.attach_bulk_metadata(n, fp.random_columns(rng, n))

    def write(tag):
        for j in range(20):                                            # inserts
            st.insert_with_metadata(f"{tag}{j}", V(rng.standard_normal(d).astype(np.float32)), M(fp.random_metadata(rng)))
        for j in range(0, 20, 4):                                      # upserts of inserted rows, and of a bulk-attached one
            st.insert_with_metadata(f"{tag}{j}", V(rng.standard_normal(d).astype(np.float32)), M(fp.random_metadata(rng)))
        st.insert_with_metadata(str(40 if tag == "a" else 41), V(rng.standard_normal(d).astype(np.float32)), M({"color": "red", "shape": "round"}))
        for j in (1, 2, 3):                                            # deletes: inserted rows and bulk-attached ones
            st.delete(f"{tag}{j}")
        for i in rng.choice(np.arange(100, n), size=15, replace=False):
            if st._present[int(i)]:
                st.delete(str(int(i)))

    write("a")
    queries = [(V(q), k) for q in qs]
    filters = store_filters(F)
    assert st.filter_program(filters["over the limit"]) is None

    def run_all():
        out = {}
        for sparse in (0, 1):                                          # the walk; the filter scan (every filter here leaves < 131072 nodes)
            st.set_sparse_filter(sparse)
            for name, flt in filters.items():
                out[(sparse, name)] = as_arrays(st.search_batch_prefiltered(queries, flt))
        st.set_sparse_filter(0)
        return out

    assert not st.device_filter()
    off = run_all()
    st.set_device_filter(True)
    assert st.device_filter()                                          # an HNSW store no longer ignores the setting
    for name, flt in filters.items():
        if name != "over the limit":
            want, bits = st.compile_filter(flt)
            with st.compile_filter_device(flt) as cm:
                got, _ = read_mask(cm)
                assert cm.bits == bits and np.array_equal(got, want), name
    on = run_all()
    assert on == off
    assert all(len(i) == k for i in on[(1, "eq")][0]) and all(len(i) == 0 for s in (0, 1) for i in on[(s, "nobody")][0])
    write("b")                                                         # writes forwarded to the resident table
    on2 = run_all()
    from starlette.testclient import TestClient
    from vectordb_from_scratch_amd.server import AppState, create_app
    client = TestClient(create_app(AppState(st)))
    body = {"queries": [{"vector": q.tolist(), "k": k} for q in qs], "filter": {"op": "eq", "field": "color", "value": "red"}, "prefilter": True}
    served_on = client.post("/search/batch", json=body)
    st.set_device_filter(False)
    assert not st.device_filter()
    assert run_all() == on2
    served_off = client.post("/search/batch", json=body)
    assert served_on.status_code == 200 and served_off.status_code == 200 and served_on.json() == served_off.json()
    assert [[x["id"] for x in hits] for hits in served_on.json()] == on2[(0, "eq")][0]


# ------------------------------------------------------------------ 6. refusals
def test_refusals(vdb):
    T, F = vdb.MetaTable, vdb.MetadataFilter
    L = vdb._ffi.lib()
    rng = np.random.default_rng(1)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 16, 16), seed=1)
    g.build_batch((np.arange(40, dtype=np.uint64), rng.standard_normal((40, 4)).astype(np.float32)))
    q = np.ones((1, 4), dtype=np.float32)
    ids, ds, cnt = np.zeros(1, np.uint64), np.zeros(1, np.float32), np.zeros(1, np.uintp)
    fpt, u64p, szp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
    before = g.stats()
    rc = L.vdb_hnsw_search_batch_filtered(g._h, q.ctypes.data_as(fpt), 1, 4, 1, 16, None, ids.ctypes.data_as(u64p), ds.ctypes.data_as(fpt),
                                          cnt.ctypes.data_as(szp))
    assert rc == vdb._ffi.ERR_INVALID_ARGUMENT and g.stats() == before
    nw, c = ctypes.c_size_t(), ctypes.c_uint64()
    assert L.vdb_hnsw_debug_present_mask(g._h, None, None, 0, ctypes.byref(nw), ctypes.byref(c)) == vdb._ffi.ERR_INVALID_ARGUMENT
    table = table_of(vdb, np.ones(40, dtype=bool))
    with table.compile([(T.CONST, 0, 1)], 40) as cm:
        with pytest.raises(ValueError):
            g.search_batch_arrays(q, 2, 16, id_mask=np.ones(1, np.uint64), mask_bits=40, compiled_mask=cm)
        with pytest.raises(ValueError):
            g.search_batch([(vdb.Vector(q[0]), 2)], id_mask=np.ones(1, np.uint64), mask_bits=40, compiled_mask=cm)
        assert g.search_batch_arrays(q, 2, 16, compiled_mask=cm)[2][0] == 2
    # a mask whose table set_device_filter(False) closed: refused by the wrapper, never handed down
    st = vdb.VectorStore.with_index(g)
    st.attach_bulk_metadata(40, {"color": np.array(["red", "blue"] * 20, dtype=object)})
    st.set_device_filter(True)
    stale = st.compile_filter_device(F.Eq("color", "red"))
    st.set_device_filter(False)
    before = g.stats()
    with pytest.raises(ValueError):
        g.search_batch_arrays(q, 2, 16, compiled_mask=stale)
    with pytest.raises(ValueError):
        g.debug_present_mask(stale)
    assert g.stats() == before
    for read in (lambda: stale.bits, lambda: stale.ptr, stale.count, lambda: stale.handle):     # nothing of a freed mask is read
        with pytest.raises(ValueError):
            read()
    flat = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)          # the flat wrapper refuses it the same way
    flat.add_bulk(np.ones((3, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        flat.search_batch_arrays(q, 2, compiled_mask=stale)
    stale.release()
    table.close()


def test_mask_of_another_device_is_refused(vdb):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    table = vdb.MetaTable(1)
    table.set_present(0, 3, True)
    g = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(4, 16, 16), device=0)
    g.build_batch((np.arange(3, dtype=np.uint64), np.eye(3, 2, dtype=np.float32) + 1))
    with table.compile([(vdb.MetaTable.CONST, 0, 1)], 3) as cm:
        with pytest.raises(vdb.VectorDbError):
            g.search_batch_arrays(np.ones((1, 2), dtype=np.float32), 2, compiled_mask=cm)
    table.close()

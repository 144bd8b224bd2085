"""Metadata filters compiled on the device (include/vdb_flat.h vdb_meta_table, csrc/kernels_filter.hip): the
store's columns and presence bitmap live in HBM, a filter becomes a postfix program and ONE kernel writes the id bitmask.

Every device mask is compared word for word with `VectorStore.compile_filter` (numpy) on the same store, the eligible count with
the mask's popcount, and every search under a compiled mask with the same search under the host mask (arrays identical) and
with the CPU oracle under that mask."""
import ctypes
import os

import numpy as np
import pytest

import filter_programs as fp
import oracle
from conftest import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


_hip = None


def read_mask(cm):
    """(the mask's words copied to the host, its eligible count); count() waits for the compile first"""
    global _hip
    count = cm.count()
    if _hip is None:
        import torch
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        _hip = ctypes.CDLL(path if os.path.exists(path) else "libamdhip64.so")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.full((cm.bits + 63) // 64, 0xdeadbeef, dtype=np.uint64)
    if out.size:
        assert cm.ptr
        assert _hip.hipMemcpy(out.ctypes.data, cm.ptr, out.size * 8, 2) == 0             # hipMemcpyDeviceToHost
    return out, count


def popcount(words):
    return int(np.unpackbits(words.view(np.uint8)).sum())


def check_store(st, filters):
    """compile_filter_device == compile_filter for every filter, on the store as it is now"""
    for f in filters:
        want, bits = st.compile_filter(f)
        with st.compile_filter_device(f) as cm:
            assert cm.bits == bits
            got, count = read_mask(cm)
        assert np.array_equal(got, want), (f.op, f.field, f.value, np.flatnonzero(got != want)[:5])
        assert count == popcount(want)


def basic_filters(F):
    return [F.Eq("color", "red"), F.Ne("color", "green"), F.Exists("color"), F.Eq("size", "m"), F.Ne("size", "m"), F.Exists("size"),
            F.Eq("shape", "round"), F.Ne("shape", "round"), F.Exists("shape"),
            F.Ne(fp.ABSENT_FIELD, "x"), F.Eq(fp.ABSENT_FIELD, "x"), F.Exists(fp.ABSENT_FIELD),        # an unknown field
            F.Eq("size", fp.ABSENT_VALUE), F.Ne("size", fp.ABSENT_VALUE),                          # a value not in the dictionary
            F.And([]), F.Or([]),
            F.And([F.Ne("color", "red"), F.Or([F.Exists("size"), F.Eq("shape", "square")])]),
            F.Or([F.And([F.Eq("color", "blue"), F.Ne("size", "s")]), F.And([]), F.Exists("shape")])]


# ------------------------------------------------------------------ 1. mask bits, column lengths, every op
@pytest.mark.parametrize("bits", [1, 63, 64, 65, 127, 4097, 70001])
def test_mask_bits_and_short_columns(vdb, bits):
    """Three device columns of lengths 0, bits // 2 and bits under a mask of `bits` ids: the first reads -1 everywhere, the second
    -1 from the middle on, without touching memory.  The expected mask is compile_filter's on a host store whose columns hold -1
    in exactly those places."""
    F = vdb.MetadataFilter
    rng = np.random.default_rng(bits)
    half = bits // 2
    cols = fp.random_columns(rng, bits)
    cols["color"][:] = None
    cols["size"][half:] = None
    if bits > 1:
        cols["size"][0], cols["shape"][bits - 1] = "m", "round"
    st = fp.host_store(vdb)
    st.attach_bulk_metadata(bits, cols)
    for i in rng.choice(bits, size=min(bits // 3, 50), replace=False):
        st.delete(str(int(i)))                                                        # holes in the presence bitmap
    assert st._next_id == bits
    table = vdb.MetaTable(0)
    slot = st._slots
    table.set_codes(slot["color"], 0, np.zeros(0, dtype=np.int32))                        # known, never written: length 0
    table.set_codes(slot["size"], 0, st._cols["size"].codes[:half])
    table.set_codes(slot["shape"], 0, st._cols["shape"].codes[:bits])
    pres = st._present[:bits]
    for i in np.flatnonzero(pres):
        table.set_present(int(i), 1, True)
    for f in basic_filters(F) + [F.Eq("color", ""), F.Ne("color", "")]:                 # ("" is in color's dictionary: real leaves on the empty column)
        want, wbits = st.compile_filter(f)
        assert wbits == bits
        with table.compile(st.filter_program(f), bits) as cm:
            got, count = read_mask(cm)
        assert got.size == (bits + 63) // 64 and np.array_equal(got, want), (bits, f.op, f.field, f.value)
        assert count == popcount(want)
        if bits % 64:
            assert int(got[-1]) >> (bits % 64) == 0                                    # the tail of the last word is clear
    # a mask SHORTER than the columns and the bitmap: ids at and above mask_bits contribute nothing
    short = max(bits - 3, 0)
    with table.compile(st.filter_program(F.And([])), short) as cm:
        got, count = read_mask(cm)
        want = fp.interpret([(fp.CONST, 0, 1)], {}, pres, short)[0]
        assert cm.bits == short and np.array_equal(got, want) and count == int(pres[:short].sum())
    table.close()


def test_random_trees_at_5000_ids(vdb):
    F = vdb.MetadataFilter
    rng = np.random.default_rng(5)
    n = 5000
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)
    ix.add_bulk(rng.standard_normal((n, 2)).astype(np.float32))
    st = vdb.VectorStore(index=ix)
    st.attach_bulk_metadata(n, fp.random_columns(rng, n))
    for i in rng.choice(n, size=400, replace=False):
        st.delete(str(int(i)))
    st.set_device_filter(True)
    assert st.device_filter()
    trees = fp.random_trees(F)
    assert len(trees) == 300
    check_store(st, trees)
    st.set_device_filter(False)
    assert not st.device_filter()
    with pytest.raises(ValueError):
        st.compile_filter_device(trees[0])


# ------------------------------------------------------------------ 2. staging: every kind of write, a compile after each
def test_staged_writes_reach_the_next_compile(vdb):
    F, M, V = vdb.MetadataFilter, vdb.Metadata, vdb.Vector
    rng = np.random.default_rng(9)
    filters = basic_filters(F)
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    st.set_device_filter(True)                                                        # enabled on an empty store: no field has a slot yet
    check_store(st, filters)
    for step in range(40):                                                            # single inserts; fields appear one after the other
        st.insert_with_metadata(f"v{step}", V([float(step), 1.0]), M(fp.random_metadata(rng) if step else {"color": "red"}))
        check_store(st, filters[:6] if step % 8 else filters)
    assert set(st._slots) == set(fp.FIELDS)
    old = st._id_to_internal["v3"]
    st.insert_with_metadata("v3", V([3.5, 1.0]), M({"color": "green", "size": "xl"}))  # an upsert: the old id's bit clears, the new one's sets
    new = st._id_to_internal["v3"]
    check_store(st, filters)
    with st.compile_filter_device(F.And([])) as cm:
        m, _ = read_mask(cm)
    assert new != old and not (int(m[old >> 6]) >> (old & 63)) & 1 and (int(m[new >> 6]) >> (new & 63)) & 1
    st.delete("v7")
    gone = 7
    check_store(st, filters)
    with st.compile_filter_device(F.And([])) as cm:
        m, count = read_mask(cm)
    assert not (int(m[gone >> 6]) >> (gone & 63)) & 1 and count == len(st) == 39
    n = 3000                                                                          # a bulk range after enabling (the columns grow past their first allocation)
    st.index().add_bulk(rng.standard_normal((n, 2)).astype(np.float32), first_id=st._next_id)
    st.attach_bulk_metadata(n, fp.random_columns(rng, n))
    check_store(st, filters)
    st.insert_with_metadata("late", V([0.0, 0.0]), M({fp.ABSENT_FIELD: "heavy", "color": "blue"}))   # a NEW field after enabling
    check_store(st, filters + [F.Eq(fp.ABSENT_FIELD, "heavy"), F.Ne(fp.ABSENT_FIELD, "heavy"), F.Exists(fp.ABSENT_FIELD)])
    with st.compile_filter_device(F.Eq(fp.ABSENT_FIELD, "heavy")) as cm:
        assert cm.count() == 1
    st.delete(str(st._bulk[0][0] + 5))                                                # a bulk-attached row
    check_store(st, filters)

    # enabling on a store that already holds rows and a bulk range
    st2 = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    for step in range(30):
        st2.insert_with_metadata(f"w{step % 25}", V([float(step), 2.0]), M(fp.random_metadata(rng)))
    st2.index().add_bulk(rng.standard_normal((2000, 2)).astype(np.float32), first_id=st2._next_id)
    st2.attach_bulk_metadata(2000, fp.random_columns(rng, 2000))
    st2.delete("w4")
    st2.set_device_filter(True)
    check_store(st2, filters)
    st2.insert_with_metadata("w4", V([1.0, 2.0]), M({"shape": "round"}))
    check_store(st2, filters)


# ------------------------------------------------------------------ 3. searches under a compiled mask
N, D, B = 20000, 64, 9


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2024)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    ks = rng.integers(1, 21, B)
    ks[0], ks[1] = 1, 20
    half = np.where(rng.random(N) < 0.5, "a", "b").astype(object)
    rare = np.full(N, None, dtype=object)
    rare[rng.choice(N, size=N // 100, replace=False)] = "y"
    return dict(rows=rows, q=q, ks=ks, cols={"half": half, "rare": rare}, oracle={})


def search_filters(F):
    return {"50%": F.Eq("half", "a"), "1%": F.Eq("rare", "y"), "0 rows": F.And([F.Eq("half", "a"), F.Eq("half", "b")])}


def make_store(vdb, data, metric, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(data["rows"])
    st = vdb.VectorStore(index=ix)
    st.attach_bulk_metadata(N, data["cols"])
    return st


def as_arrays(results):
    """[[SearchResult]] -> (ids per query, distance bits per query)"""
    return [[r.id for r in res] for res in results], [np.array([r.distance for r in res], dtype=np.float32).view(np.uint32).tolist() for res in results]


def check_against_oracle(data, metric, name, st, flt, got):
    key = (metric, name)
    if key not in data["oracle"]:                                                     # computed once per (metric, filter), shared by the index kinds
        mask, bits = st.compile_filter(flt)
        live = np.unpackbits(mask.view(np.uint8), bitorder="little")[:N].astype(np.uint8)
        data["oracle"][key] = [oracle.flat_search(metric, data["rows"], data["q"][b], int(data["ks"][b]), live=live) for b in range(B)]
    ids, bitsd = got
    for b, (oi, od) in enumerate(data["oracle"][key]):
        assert ids[b] == [str(int(i)) for i in oi], (metric, name, b)
        assert bitsd[b] == od.view(np.uint32).tolist(), (metric, name, b)


@pytest.mark.parametrize("kind", ["plain", "sparse", "2 shards"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_prefiltered_search_on_equals_off_and_the_oracle(vdb, data, metric, kind):
    F = vdb.MetadataFilter
    st = make_store(vdb, data, metric, **({"devices": [0, 0]} if kind == "2 shards" else {}))
    if kind == "sparse":
        st.set_sparse_filter(1)
    queries = [(vdb.Vector(data["q"][b]), int(data["ks"][b])) for b in range(B)]
    for name, flt in search_filters(F).items():
        st.set_device_filter(False)
        off = as_arrays(st.search_batch_prefiltered(queries, flt))
        st.set_device_filter(True)
        with st.compile_filter_device(flt) as cm:
            eligible = cm.count()
        assert {"50%": 0.45 * N < eligible < 0.55 * N, "1%": eligible == N // 100, "0 rows": eligible == 0}[name]
        on = as_arrays(st.search_batch_prefiltered(queries, flt))
        assert on == off, (metric, kind, name)
        assert [len(i) for i in on[0]] == [min(int(k), eligible) for k in data["ks"]]
        if kind == "sparse":
            assert st.index().sparse_stats()[0] == 1 and st.index().sparse_stats()[1] == eligible     # the route really answered
        check_against_oracle(data, metric, name, st, flt, on)


def test_mask_pointer_in_the_device_resident_search(vdb, data):
    import torch
    F = vdb.MetadataFilter
    st = make_store(vdb, data, 0)
    st.set_device_filter(True)
    ix, k = st.index(), 10
    dev = torch.device("cuda:0")
    q_t = torch.from_numpy(data["q"]).to(dev)
    side = torch.cuda.Stream(dev)                                                     # a stream of the caller's own (not the null stream)
    for name, flt in search_filters(F).items():
        mask, bits = st.compile_filter(flt)
        m_t = torch.from_numpy(mask.view(np.int64)).to(dev)
        outs = []
        for use_compiled in (False, True):
            o_i = torch.zeros((B, k), dtype=torch.int64, device=dev)
            o_d = torch.zeros((B, k), dtype=torch.float32, device=dev)
            o_c = torch.zeros(B, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            if use_compiled:
                stream = side.cuda_stream
                with st.compile_filter_device(flt) as cm:
                    assert cm.bits == bits
                    cm.wait_on(stream)                                                 # no host wait: the stream is ordered behind the mask
                    ix.search_batch_device(q_t.data_ptr(), B, D, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), stream=stream,
                                           mask_ptr=cm.ptr, mask_bits=cm.bits)
            else:
                ix.search_batch_device(q_t.data_ptr(), B, D, k, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mask_ptr=m_t.data_ptr(), mask_bits=bits)
            torch.cuda.synchronize()
            outs.append((o_i.cpu().numpy(), o_d.cpu().numpy().view(np.uint32), o_c.cpu().numpy()))
        for x, y in zip(*outs):
            assert np.array_equal(x, y), name
        assert (outs[1][2] == min(k, popcount(mask))).all()


# ------------------------------------------------------------------ 4. limits, refusals, the pool
def test_over_limit_program_falls_back_to_the_host_mask(vdb, data):
    F = vdb.MetadataFilter
    st = make_store(vdb, data, 0)
    queries = [(vdb.Vector(data["q"][b]), int(data["ks"][b])) for b in range(B)]
    big = F.Or([F.Eq("rare", "y")] * 513)                                             # 1025 ops
    deep = F.Eq("rare", "y")
    for _ in range(32):
        deep = F.And([F.Exists("half"), deep])                                        # stack depth 33
    want = as_arrays(st.search_batch_prefiltered(queries, F.Eq("rare", "y")))
    st.set_device_filter(True)
    for flt in (big, deep):
        assert st.filter_program(flt) is None and st.compile_filter_device(flt) is None
        assert as_arrays(st.search_batch_prefiltered(queries, flt)) == want
    check_against_oracle(data, 0, "1%", st, F.Eq("rare", "y"), want)
    ok = F.Or([F.Eq("rare", "y")] * 512)                                              # 1023 ops: the longest Or that fits, on the device
    assert len(st.filter_program(ok)) == 1023
    check_store(st, [ok])
    assert as_arrays(st.search_batch_prefiltered(queries, ok)) == want


def test_refusals(vdb):
    T = vdb.MetaTable
    L = vdb._ffi.lib()
    table = T(0)
    table.set_codes(0, 0, np.array([0, 1, -1], dtype=np.int32))
    table.set_present(0, 3, True)
    leaf = (T.EXISTS, 0, 0)
    bad = {
        "1025 ops": [leaf] + [leaf, (T.OR, 0, 0)] * 512,
        "depth 33": [leaf] * 33 + [(T.AND, 0, 0)] * 32,
        "unknown slot": [(T.EQ, 5, 0)],
        "AND with one operand": [leaf, (T.AND, 0, 0)],
        "two values left": [leaf, leaf],
        "empty": [],
        "CONST 2": [(T.CONST, 0, 2)],
        "opcode 9": [(9, 0, 0)],
    }
    for name, prog in bad.items():
        with pytest.raises(vdb.VectorDbError):
            table.compile(prog, 3)
    for prog in ([leaf] + [leaf, (T.OR, 0, 0)] * 511, [leaf] * 32 + [(T.AND, 0, 0)] * 31):   # 1023 ops / depth 32: the limits themselves pass
        with table.compile(prog, 3) as cm:
            got, count = read_mask(cm)
        assert got.tolist() == [0b011] and count == 2
    with table.compile([leaf], 0) as cm:                                              # mask_bits == 0: nothing is written, nothing counted
        assert cm.bits == 0 and cm.count() == 0
    for call in (lambda: table.set_codes(0, 1 << 32, np.zeros(1, dtype=np.int32)), lambda: table.set_codes(0, (1 << 32) - 1, np.zeros(2, dtype=np.int32)),
                 lambda: table.set_present(1 << 32, 1, True), lambda: table.set_present((1 << 32) - 1, 2, True)):
        with pytest.raises(vdb.VectorDbError):
            call()
    # a null mask
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)
    ix.add_bulk(np.ones((3, 2), dtype=np.float32))
    q = np.ones((1, 2), dtype=np.float32)
    ids, ds, cnt = np.zeros(1, np.uint64), np.zeros(1, np.float32), np.zeros(1, np.uintp)
    fpt, u64p, szp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_size_t)
    rc = L.vdb_flat_search_batch_filtered(ix._h, q.ctypes.data_as(fpt), 1, 2, None, 1, None, 1, ids.ctypes.data_as(u64p), ds.ctypes.data_as(fpt),
                                          cnt.ctypes.data_as(szp))
    assert rc == vdb._ffi.ERR_INVALID_ARGUMENT
    with table.compile([(T.EQ, 0, 1)], 3) as cm:                                      # and a real one on the same handle: id 1 only
        gi, gd, gc = ix.search_batch_arrays(q, 2, compiled_mask=cm)
        assert gc.tolist() == [1] and gi[0, 0] == 1
        with pytest.raises(ValueError):
            ix.search_batch_arrays(q, 2, id_mask=np.ones(1, np.uint64), mask_bits=3, compiled_mask=cm)
    table.close()


def test_mask_of_another_device_is_refused(vdb):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    table = vdb.MetaTable(1)
    table.set_present(0, 3, True)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, device=0, keep_host_copy=False)
    ix.add_bulk(np.ones((3, 2), dtype=np.float32))
    with table.compile([(vdb.MetaTable.CONST, 0, 1)], 3) as cm:
        with pytest.raises(vdb.VectorDbError):
            ix.search_batch_arrays(np.ones((1, 2), dtype=np.float32), 2, compiled_mask=cm)
    table.close()


def test_pool_reuses_a_released_buffer(vdb):
    T = vdb.MetaTable
    table = T(0)
    table.set_present(0, 1000, True)
    prog = [(T.CONST, 0, 1)]
    a = table.compile(prog, 1000)
    b = table.compile(prog, 1000)                                                     # both outstanding: two buffers
    pa, pb = a.ptr, b.ptr
    assert pa and pb and pa != pb
    assert a.count() == 1000 and b.count() == 1000
    a.release()
    c = table.compile(prog, 900)                                                      # the released buffer again, no allocation
    assert c.ptr == pa and c.count() == 900
    with pytest.raises(ValueError):
        a.ptr                                                                         # the wrapper of a released mask refuses to be used
    b.release()
    c.release()
    table.close()

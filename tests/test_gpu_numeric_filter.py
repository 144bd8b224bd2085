"""Numeric range predicates on the device (MetadataFilter.Lt / Le / Gt / Ge -> VDB_META_LT .. GE, vdb_meta_set_numbers,
vdb_meta_compile_num, the numeric leaf of csrc/kernels_filter.hip).

Every device mask is compared word for word and in count with the numpy interpreter of tests/numeric_filter_programs.py (raw
tables: any int32 in a column, any LUT length) or with `VectorStore.compile_filter` (stores), and every search route under a
compiled numeric mask with the same route under the host mask and with the CPU oracle."""
import ctypes

import numpy as np
import pytest

import filter_programs as fp
import numeric_filter_programs as nfp
import oracle
from conftest import load_package
from test_gpu_device_filter import as_arrays, popcount, read_mask

pytestmark = pytest.mark.gpu

INF = float("inf")
TWO53 = 2.0 ** 53
ONE_UP, ONE_DOWN = float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0))
# what a LUT may hold: +-0, subnormals, neighbours one ulp apart, 2^53, huge values, NaN ("no number")
LUT_VALUES = np.array([1.0, np.nan, -0.0, 0.0, nfp.TINY, -nfp.TINY, ONE_UP, ONE_DOWN, TWO53, -1e300, 1e300, np.nan, 2.5e-310, -3.5, 1.0, 99.0], dtype=np.float64)
CONSTANTS = [0.0, -0.0, INF, -INF, nfp.TINY, 2.5e-310, 1.0, ONE_UP, ONE_DOWN, TWO53]
OPS = (nfp.LT, nfp.LE, nfp.GT, nfp.GE)


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def check_program(table, prog, consts, columns, luts, present, bits):
    want, count = nfp.interpret(prog, consts, columns, luts, present, bits)
    with table.compile(prog, bits, consts) as cm:
        got, n = read_mask(cm)
    assert got.size == (bits + 63) // 64
    assert np.array_equal(got, want), (prog[:4], consts[:4], bits, np.flatnonzero(got != want)[:5])
    assert n == count == popcount(want)
    if bits % 64:
        assert int(got[-1]) >> (bits % 64) == 0
    return count


# ------------------------------------------------------------------ 1. the kernel against the interpreter
@pytest.mark.parametrize("bits", [1, 63, 64, 65, 127, 4097, 70001])
def test_kernel_equals_interpreter(vdb, bits):
    """Six columns under a mask of `bits` ids.  0: full length, codes -1 .. 39, LUT of 30 (shorter than the largest code).
    1: half the mask long, LUT of length 1.  2: known, empty, with a LUT.  3: ANY int32 -- -1, -7, 2^31 - 1, codes beyond the LUT --
    written through the raw table, LUT of 6.  4: codes, and a LUT of length 0 (set_numbers with n = 0).  5: codes, no LUT at all.
    The bounds check in front of the LUT read is what keeps column 3 inside its table: the result must be the interpreter's."""
    rng = np.random.default_rng(100 + bits)
    half = bits // 2
    weird = np.array([-1, -7, 2 ** 31 - 1, 0, 1, 5, 6, 1000, -2 ** 31, 3], dtype=np.int32)
    columns = {0: rng.integers(-1, 40, bits).astype(np.int32), 1: rng.integers(-1, 3, half).astype(np.int32), 2: np.zeros(0, dtype=np.int32),
               3: weird[rng.integers(0, weird.size, bits)], 4: rng.integers(-1, 4, bits).astype(np.int32), 5: rng.integers(-1, 4, bits).astype(np.int32)}
    luts = {0: np.resize(LUT_VALUES, 30), 1: LUT_VALUES[:1], 2: LUT_VALUES[:5], 3: LUT_VALUES[:6], 4: np.zeros(0)}
    present = rng.random(bits) < 0.9
    table = vdb.MetaTable(0)
    for slot, codes in columns.items():
        table.set_codes(slot, 0, codes)
    for slot, lut in luts.items():
        table.set_numbers(slot, 0, lut)
    for a, b in zip(*[iter(np.flatnonzero(np.diff(np.concatenate(([False], present, [False])).astype(np.int8))))] * 2):
        table.set_present(int(a), int(b - a), True)
    some = 0
    for slot in columns:
        for op in OPS:                                                      # one program per (column, op): an OR over every constant ...
            prog = [(op, slot, 0)]
            for j in range(1, len(CONSTANTS)):
                prog += [(op, slot, j), (nfp.OR, 0, 0)]
            check_program(table, prog, CONSTANTS, columns, luts, present, bits)
        for j, c in enumerate(CONSTANTS):                                   # ... and per (column, constant): lt | gt, le & ge, each alone in its word
            for prog in ([(nfp.LT, slot, 0), (nfp.GT, slot, 0), (nfp.OR, 0, 0)], [(nfp.LE, slot, 0), (nfp.GE, slot, 0), (nfp.AND, 0, 0)],
                         [(nfp.LT, slot, 0)], [(nfp.GE, slot, 0)]):
                some += check_program(table, prog, [c], columns, luts, present, bits)
    if bits > 100:
        assert some > 0
    # mixed with string leaves and a constant, over columns of different lengths
    prog = [(nfp.GE, 0, 0), (fp.EQ, 1, 1), (fp.OR, 0, 0), (nfp.LT, 3, 1), (fp.NE, 4, 2), (fp.AND, 0, 0), (fp.OR, 0, 0), (fp.EXISTS, 2, 0), (fp.OR, 0, 0),
            (fp.CONST, 0, 1), (fp.AND, 0, 0), (nfp.GT, 5, 2), (fp.OR, 0, 0)]
    check_program(table, prog, [1.0, INF, -INF], columns, luts, present, bits)
    # a mask SHORTER than the columns: ids at and above mask_bits contribute nothing
    check_program(table, [(nfp.GT, 0, 0)], [-INF], columns, luts, present, max(bits - 3, 0))
    # Gt(-inf) is "has a number": on column 0 exactly the present ids whose code names a non-NaN LUT entry
    c0 = columns[0]
    has = (c0 >= 0) & (c0 < 30)
    has[has] = ~np.isnan(luts[0][c0[has]])
    assert check_program(table, [(nfp.GT, 0, 0)], [-INF], columns, luts, present, bits) == int((has & present).sum())
    table.close()


# ------------------------------------------------------------------ 2. random trees on a store
def gpu_store(vdb, rng, device_filter_first):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric.Euclidean, keep_host_copy=False)
    st = vdb.VectorStore(index=ix)
    if device_filter_first:
        st.set_device_filter(True)                                          # every write below is forwarded, the LUT tails included
    nfp.build_store(vdb, st, rng, add_rows=lambda first, n: ix.add_bulk(rng.standard_normal((n, 2)).astype(np.float32), first_id=first))
    return st


def check_store(st, filters):
    for f in filters:
        want, bits = st.compile_filter(f)
        with st.compile_filter_device(f) as cm:
            assert cm.bits == bits
            got, count = read_mask(cm)
        assert np.array_equal(got, want), (f.op, f.field, f.value, np.flatnonzero(got != want)[:5])
        assert count == popcount(want)


def test_random_trees_at_5000_ids(vdb):
    F = vdb.MetadataFilter
    trees = nfp.random_trees(F)
    assert len(trees) == 300
    st = gpu_store(vdb, np.random.default_rng(31), device_filter_first=True)
    assert st._next_id == 5000 and st.device_filter()
    check_store(st, trees)
    st.set_device_filter(False)
    st.set_device_filter(True)                                              # the whole table again, LUTs included, in one go
    check_store(st, trees[:100])
    st.insert_with_metadata("late", vdb.Vector([0.0, 0.0]), vdb.Metadata({"price": "12345.5", "score": "-7e-3", "rating": "4.5"}))   # new codes, a new field
    check_store(st, trees[:40] + [F.Gt("price", 12345.0), F.Le("score", -7e-3), F.Ge("rating", 4.5), F.Lt("rating", 4.5)])
    with st.compile_filter_device(F.Gt("price", 12345.0)) as cm:
        assert cm.count() == 1
    with st.compile_filter_device(F.Ge("rating", 4.5)) as cm:
        assert cm.count() == 1


# ------------------------------------------------------------------ 3. staged writes
def test_staged_lut_writes_and_regrows(vdb):
    """A compiled mask stays unreleased while the LUT grows past 1024 and past 2048 entries (two device regrows of the staged
    array, each behind a stream synchronisation) and the codes change; every mask holds what its own compile saw."""
    T = vdb.MetaTable
    rng = np.random.default_rng(77)
    n = 3000
    table = T(0)
    table.set_present(0, n, True)
    present = np.ones(n, dtype=bool)
    lut = rng.integers(0, 1000, 500).astype(np.float64)
    codes = rng.integers(-1, 500, n).astype(np.int32)
    table.set_codes(0, 0, codes)
    table.set_numbers(0, 0, lut)
    prog, consts = [(nfp.LT, 0, 0), (nfp.GE, 0, 1), (nfp.OR, 0, 0)], [250.0, 900.0]
    masks, wants = [], []

    def compile_and_keep():
        masks.append(table.compile(prog, n, consts))
        wants.append(nfp.interpret(prog, consts, {0: codes.copy()}, {0: lut.copy()}, present, n))
    compile_and_keep()
    for size in (1200, 2500):
        more = rng.integers(0, 1000, size - lut.size).astype(np.float64)
        table.set_numbers(0, lut.size, more)                                 # the tail only
        lut = np.concatenate([lut, more])
        at = rng.choice(n, size=n // 2, replace=False)
        codes[at] = rng.integers(0, size + 50, at.size)                      # (some beyond the LUT: no number)
        lo, hi = int(at.min()), int(at.max()) + 1
        table.set_codes(0, lo, codes[lo:hi])
        compile_and_keep()
    lut[3] = np.nan                                                          # an entry rewritten in place: a dirty range inside the LUT
    table.set_numbers(0, 3, lut[3:4])
    compile_and_keep()
    table.set_numbers(1, 0, np.array([5.0]))                                 # a LUT for a slot whose column does not exist yet: the slot stays unknown
    with pytest.raises(vdb.VectorDbError):
        table.compile([(nfp.LT, 1, 0)], n, [9.0])
    for cm, (want, count) in zip(masks, wants):
        got, c = read_mask(cm)
        assert np.array_equal(got, want) and c == count
    assert len({cm.ptr for cm in masks}) == 4 and len({w[1] for w in wants}) > 1
    for cm in masks:
        cm.release()
    table.close()


# ------------------------------------------------------------------ 4. limits and refusals
def test_limits_and_refusals(vdb):
    T = vdb.MetaTable
    L = vdb._ffi.lib()
    rng = np.random.default_rng(5)
    n = 1000
    codes = rng.integers(-1, 100, n).astype(np.int32)
    lut = np.arange(100, dtype=np.float64)
    table = T(0)
    table.set_codes(0, 0, codes)
    table.set_numbers(0, 0, lut)
    table.set_present(0, n, True)
    present = np.ones(n, dtype=bool)
    cols, luts = {0: codes}, {0: lut}
    # 1023 ops of numeric leaves, 512 distinct constants: the longest program, every leaf with its record in LDS
    consts = [float(v) for v in rng.choice(np.arange(-2, 1022) / 8.0, size=512, replace=False)]
    prog = []
    for j in range(512):
        prog.append((OPS[j % 4], 0, j))
        if j:
            prog.append((nfp.OR if j % 3 else nfp.AND, 0, 0))
    assert len(prog) == 1023
    count = check_program(table, prog, consts, cols, luts, present, n)
    assert 0 < count < n
    deep = [(nfp.GE, 0, 0)] * 32 + [(nfp.AND, 0, 0)] * 31                     # depth 32 passes
    assert check_program(table, deep, [50.0], cols, luts, present, n) == int((codes >= 50).sum())
    leaf = (nfp.LT, 0, 0)
    bad = {
        "1025 constants": ([leaf], [float(i) for i in range(1025)]),
        "constant index == n_consts": ([(nfp.LT, 0, 2)], [1.0, 2.0]),
        "constant index -1": ([(nfp.LT, 0, -1)], [1.0]),
        "a NaN constant": ([leaf], [float("nan")]),
        "a NaN constant nobody uses": ([leaf], [1.0, float("nan")]),
        "a numeric op through vdb_meta_compile": ([leaf], None),
        "no constants at all": ([leaf], []),
        "unknown slot": ([(nfp.GT, 7, 0)], [1.0]),
        "opcode 9": ([(9, 0, 0)], [1.0]),
        "opcode 15": ([(15, 0, 0)], [1.0]),
        "opcode 20": ([(20, 0, 0)], [1.0]),
        "depth 33": ([leaf] * 33 + [(nfp.AND, 0, 0)] * 32, [1.0]),
        "1025 ops": ([leaf] + [leaf, (nfp.OR, 0, 0)] * 512, [1.0]),
    }
    for name, (p, c) in bad.items():
        with pytest.raises(vdb.VectorDbError):
            table.compile(p, n, c)
    ops = (vdb._ffi.MetaOp * 1)()
    ops[0].op, ops[0].slot, ops[0].code = nfp.LT, 0, 0
    m = ctypes.c_void_p()
    assert L.vdb_meta_compile_num(table._t, ops, 1, None, 1, n, ctypes.byref(m)) == vdb._ffi.ERR_INVALID_ARGUMENT and not m.value   # null consts
    for call in (lambda: table.set_numbers(0, 1 << 31, np.ones(1)), lambda: table.set_numbers(0, (1 << 31) - 1, np.ones(2)),
                 lambda: table.set_numbers(1 << 16, 0, np.ones(1))):
        with pytest.raises(vdb.VectorDbError):
            call()
    table.set_numbers(0, 1 << 31, np.zeros(0))                                # n = 0 is allowed, also at the end of the code space
    assert L.vdb_abi_version() == 1
    # the table is as usable as before: 1024 constants fit, and a program without numeric leaves takes either entry
    assert check_program(table, [(nfp.LE, 0, 1023)], [0.0] * 1023 + [9.0], cols, luts, present, n) == int(((codes >= 0) & (codes <= 9)).sum())
    for c in (None, []):
        with table.compile([(fp.EXISTS, 0, 0)], n, c) as cm:
            assert cm.count() == int((codes >= 0).sum())
    table.close()


# ------------------------------------------------------------------ 5. every consumer
N, D, B, K = 6000, 32, 8, 10


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(606)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((B, D)).astype(np.float32)
    ks = rng.integers(1, 21, B)
    ks[0], ks[1] = 1, 20
    price = np.array([str(int(v)) for v in rng.integers(0, 100, N)], dtype=object)
    score = np.array([repr(float(v)) for v in np.round(rng.standard_normal(N), 3)], dtype=object)       # duplicates: about 6000 draws of a few thousand values
    score[rng.random(N) < 0.1] = None
    color = np.array(["red", "green", "blue"], dtype=object)[rng.integers(0, 3, N)]
    doc = np.array([f"d{int(v)}" for v in rng.integers(0, 400, N)], dtype=object)
    return dict(rows=rows, q=q, ks=ks, cols={"price": price, "score": score, "color": color, "doc": doc}, oracle={})


def numeric_filters(F):
    return {"lt": F.Lt("price", 25), "band": F.And([F.Ge("price", 25), F.Lt("price", 75), F.Eq("color", "red")]),
            "or": F.Or([F.Gt("score", 1.0), F.Le("price", 3)])}


def make_store(vdb, data, metric, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(data["rows"])
    st = vdb.VectorStore(index=ix)
    st.attach_bulk_metadata(N, data["cols"])
    return st


def live_of(st, flt):
    mask, bits = st.compile_filter(flt)
    assert bits == N
    return np.unpackbits(mask.view(np.uint8), bitorder="little")[:N].astype(np.uint8)


def eligible_of(st, flt):
    """the device's count, asserted strictly between k and the row count: an all-ones or all-zeros mask cannot pass"""
    with st.compile_filter_device(flt) as cm:
        e = cm.count()
    assert 20 < e < N - 20 and e == int(live_of(st, flt).sum())
    return e


def oracle_lists(data, metric, name, st, flt):
    key = (metric, name)
    if key not in data["oracle"]:                                            # once per (metric, filter), shared by the routes and index kinds
        live = live_of(st, flt)
        data["oracle"][key] = [oracle.flat_search(metric, data["rows"], data["q"][b], int(data["ks"][b]), live=live) for b in range(B)]
    return data["oracle"][key]


def assert_equals_oracle(got, lists, what):
    ids, bitsd = got
    for b, (oi, od) in enumerate(lists):
        assert ids[b] == [str(int(i)) for i in oi], (what, b)
        assert bitsd[b] == od.view(np.uint32).tolist(), (what, b)


@pytest.mark.parametrize("kind", ["plain", "sparse", "2 shards"])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_prefiltered_search_on_equals_off_and_the_oracle(vdb, data, metric, kind):
    F = vdb.MetadataFilter
    st = make_store(vdb, data, metric, **({"devices": [0, 0]} if kind == "2 shards" else {}))
    if kind == "sparse":
        st.set_sparse_filter(1)
    queries = [(vdb.Vector(data["q"][b]), int(data["ks"][b])) for b in range(B)]
    for name, flt in numeric_filters(F).items():
        st.set_device_filter(False)
        off = as_arrays(st.search_batch_prefiltered(queries, flt))
        st.set_device_filter(True)
        eligible = eligible_of(st, flt)
        on = as_arrays(st.search_batch_prefiltered(queries, flt))
        assert on == off, (metric, kind, name)
        assert [len(i) for i in on[0]] == [int(k) for k in data["ks"]]
        if kind == "sparse":
            assert st.index().sparse_stats()[0] == 1 and st.index().sparse_stats()[1] == eligible
        assert_equals_oracle(on, oracle_lists(data, metric, name, st, flt), (metric, kind, name))


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_flat_routes_on_equals_off_and_the_oracle(vdb, data, metric):
    """search_within, search_similar_batch, search_distinct_batch and search_batch_with_filters under numeric filters"""
    F, V = vdb.MetadataFilter, vdb.Vector
    st = make_store(vdb, data, metric)
    rows, q = data["rows"], data["q"]
    filters = numeric_filters(F)
    queries = [(V(q[b]), int(data["ks"][b])) for b in range(B)]
    per_query = [list(filters)[b % 3] if b != 5 else None for b in range(B)]   # a different numeric filter per query, one query without
    sim_ids = [str(i) for i in (0, 17, 4099, 5999)]
    doc_codes = np.array([int(v[1:]) for v in data["cols"]["doc"]])

    def run_all():
        out = {}
        for name, flt in filters.items():
            full = oracle.flat_search(metric, rows, q[0], 40, live=live_of(st, flt))
            radius = float(full[1][25])                                      # a radius with 26 or more rows inside: the limit of 20 cuts
            out[("within", name)] = as_arrays([st.search_within(V(q[0]), radius, 20, flt), st.search_within(V(q[1]), float(full[1][5]) * 0.5, 30, flt)])
            out[("similar", name)] = as_arrays(st.search_similar_batch(sim_ids, K, flt))
            if st.device_filter():                                           # (the collapse reads the resident column: no host-only form)
                out[("distinct", name)] = as_arrays(st.search_distinct_batch([V(q[b]) for b in range(3)], K, "doc", flt))
        out["per query"] = as_arrays(st.search_batch_with_filters(queries, [filters[n] if n else None for n in per_query]))
        return out

    off = run_all()
    st.set_device_filter(True)
    for flt in filters.values():
        eligible_of(st, flt)
    on = run_all()
    for key, val in off.items():
        assert on[key] == val, (metric, key)
    for name, flt in filters.items():
        live = live_of(st, flt)
        # search_within: the front of the oracle's ranking of the eligible rows, cut at the limit
        full = oracle.flat_search(metric, rows, q[0], 40, live=live)
        ids, bitsd = on[("within", name)]
        assert ids[0] == [str(int(i)) for i in full[0][:20]] and bitsd[0] == full[1][:20].view(np.uint32).tolist(), (metric, name)
        # search_similar_batch: the oracle's search with the stored row as the query, that row itself not eligible
        ids, bitsd = on[("similar", name)]
        for j, sid in enumerate(sim_ids):
            lv = live.copy()
            lv[int(sid)] = 0
            oi, od = oracle.flat_search(metric, rows, rows[int(sid)], K, live=lv)
            assert ids[j] == [str(int(i)) for i in oi] and bitsd[j] == od.view(np.uint32).tolist(), (metric, name, sid)
        # search_distinct_batch: the oracle's full ranking of the eligible rows, the first row of every doc, the first K of those
        ids, bitsd = on[("distinct", name)]
        for b in range(3):
            oi, od = oracle.flat_search(metric, rows, q[b], int(live.sum()), live=live)
            seen, keep = set(), []
            for r, i in enumerate(oi):
                if doc_codes[int(i)] not in seen:
                    seen.add(doc_codes[int(i)])
                    keep.append(r)
                    if len(keep) == K:
                        break
            assert ids[b] == [str(int(oi[r])) for r in keep] and bitsd[b] == od[keep].view(np.uint32).tolist(), (metric, name, b)
    ids, bitsd = on["per query"]
    for b, name in enumerate(per_query):
        if name is None:
            oi, od = oracle.flat_search(metric, rows, q[b], int(data["ks"][b]))
        else:
            oi, od = oracle_lists(data, metric, name, st, filters[name])[b]
        assert ids[b] == [str(int(i)) for i in oi] and bitsd[b] == od.view(np.uint32).tolist(), (metric, "per query", b)


def test_hnsw_store_walk_and_filter_scan_device_mask_equals_host_mask(vdb):
    F, V = vdb.MetadataFilter, vdb.Vector
    rng = np.random.default_rng(12)
    n, d, k = 2000, 16, 10
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((6, d)).astype(np.float32)
    ix = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 64, 50), seed=1)
    ix.build_batch((np.arange(n, dtype=np.uint64), rows))
    st = vdb.VectorStore.with_index(ix)
    st.attach_bulk_metadata(n, nfp.random_columns(rng, n))
    for i in rng.choice(n, size=40, replace=False):
        st.delete(str(int(i)))
    for j in range(10):
        st.insert_with_metadata(f"a{j}", V(rng.standard_normal(d).astype(np.float32)), vdb.Metadata(nfp.random_metadata(rng)))
    filters = {"lt": F.Lt("price", 25), "band": F.And([F.Ge("price", 25), F.Lt("price", 75), F.Eq("color", "red")]),
               "or": F.Or([F.Gt("score", 0.5), F.Le("price", 3)])}
    queries = [(V(q), k) for q in qs]

    def run_all():
        out = {}
        for sparse in (0, 1):                                                # the walk; the exact scan of the eligible nodes
            st.set_sparse_filter(sparse)
            for name, flt in filters.items():
                out[(sparse, name)] = as_arrays(st.search_batch_prefiltered(queries, flt))
        st.set_sparse_filter(0)
        return out

    off = run_all()
    st.set_device_filter(True)
    for name, flt in filters.items():
        want, bits = st.compile_filter(flt)
        with st.compile_filter_device(flt) as cm:
            got, count = read_mask(cm)
        assert np.array_equal(got, want) and k < count < len(st) - k, name
    on = run_all()
    assert on == off
    assert all(len(i) == k for name in filters for i in on[(1, name)][0])    # (the scan is exact; the walk may find fewer than k under a mask)
    assert all(len(i) > 0 for name in filters for i in on[(0, name)][0])


def test_search_batch_endpoint_with_a_ge_filter(vdb, data):
    from starlette.testclient import TestClient
    from vectordb_from_scratch_amd.server import AppState, create_app
    F = vdb.MetadataFilter
    st = make_store(vdb, data, 0)
    st.set_device_filter(True)
    flt = F.Ge("price", 90)
    eligible_of(st, flt)
    client = TestClient(create_app(AppState(st)))
    body = {"queries": [{"vector": data["q"][b].tolist(), "k": int(data["ks"][b])} for b in range(B)], "filter": {"op": "ge", "field": "price", "value": 90},
            "prefilter": True}
    r = client.post("/search/batch", json=body)
    assert r.status_code == 200
    want = as_arrays(st.search_batch_prefiltered([(vdb.Vector(data["q"][b]), int(data["ks"][b])) for b in range(B)], flt))
    assert [[x["id"] for x in hits] for hits in r.json()] == want[0]
    assert all(int(data["cols"]["price"][int(i)]) >= 90 for ids in want[0] for i in ids)
    assert_equals_oracle(want, oracle_lists(data, 0, "ge90", st, flt), "served")
    for bad in ("90", True):                                                 # a malformed filter: refused like any other
        r = client.post("/search/batch", json={**body, "filter": {"op": "ge", "field": "price", "value": bad}})
        assert r.status_code in (400, 422)

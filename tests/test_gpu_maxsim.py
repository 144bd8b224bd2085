"""Late-interaction (MaxSim) search (vdb_flat_search_batch_maxsim, csrc/kernels_maxsim.hip).  Every case compares
codes, order, score bits, counts and vdb_flat_maxsim_stats with the definition computed from the CPU oracle's distances
(tests/maxsim_data.py).  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import distinct_data as dd
import maxsim_data as md
from conftest import load_package
from split_schedule import F32 as LAYOUT_F32, SPLIT

pytestmark = pytest.mark.gpu
F32, U64, I32 = np.float32, np.uint64, np.int32


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def make_index(vdb, metric, rows, ids=None, **kw):
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
    ix.add_bulk(rows, ids=ids)
    return ix


def make_table(vdb, codes):
    t = vdb.MetaTable(0)
    t.set_codes(0, 0, np.ascontiguousarray(codes, dtype=I32))
    t.set_present(0, len(codes), True)                                         # (what a compiled mask ANDs in)
    return t


def setup(vdb, metric, n, dim, name, rows=None):
    """(rows, codes by row, n_codes, index, table) of a layout of tests/maxsim_data.py"""
    rows = md.rows(n, dim) if rows is None else rows
    codes, n_codes = md.layout(name, n)
    return rows, codes, n_codes, make_index(vdb, metric, rows), make_table(vdb, codes)


def run_and_check(ix, t, metric, rows, row_codes, n_codes, toks, k, ok=None, chunks=1, what="", **kw):
    got = ix.search_batch_maxsim(toks, k, t, 0, n_codes, **kw)
    want = md.expected(metric, rows, row_codes, toks, k, ok=ok)
    md.check(got, want, what)
    assert ix.maxsim_stats() == md.stats(row_codes, toks, want, chunks=chunks, ok=ok), (what, ix.maxsim_stats())
    return got


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("dim", [20, 33, 64, 100])
@pytest.mark.parametrize("metric", md.METRICS)
def test_every_token_count_in_one_call(vdb, metric, dim, n):
    rows, codes, n_codes, ix, t = setup(vdb, metric, n, dim, "mixed")
    run_and_check(ix, t, metric, rows, codes, n_codes, md.tokens(dim), 12, what=(metric, dim, n))


@pytest.mark.parametrize("name", md.LAYOUTS)
def test_document_shapes_per_query_k_and_k_above_the_documents(vdb, name):
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 1000, 33, name)
    ks = np.array([3, 100, 1, 0, 17, 1024, 64])                                # (all but `single` hold fewer than 100 documents)
    got = run_and_check(ix, t, md.EUCLID, rows, codes, n_codes, md.tokens(33), ks, what=name)
    assert got[2][3] == 0 and got[2][5] == min(1024, np.unique(codes[codes >= 0]).size)


def test_rows_without_a_code_and_ids_beyond_the_column_are_no_documents(vdb):
    n, dim, metric = 1000, 20, md.COSINE
    rows = md.rows(n, dim)
    ids = (np.arange(n, dtype=U64) * U64(7)) % U64(1500)                       # distinct; a third of them at or beyond the column
    column, n_codes = md.layout("mixed", 1000)
    row_codes = dd.codes_of(ids, column)
    assert np.unique(ids).size == n and (row_codes == -1).sum() > 250 and (ids >= 1000).any()
    run_and_check(make_index(vdb, metric, rows, ids=ids), make_table(vdb, column), metric, rows, row_codes, n_codes, md.tokens(dim, (2, 32)), 50)


def test_host_mask_compiled_mask_and_a_mask_that_removes_a_best_row(vdb):
    n, metric = 1000, md.EUCLID
    rows, codes, n_codes, ix, t = setup(vdb, metric, n, 33, "adjacent")
    toks = md.tokens(33, (4, 17))
    ok = np.arange(n) % 3 != 1
    mask, bits = dd.id_mask(ok)
    a = run_and_check(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, id_mask=mask, mask_bits=bits, what="host mask")
    t.set_codes(1, 0, (np.arange(n) % 3).astype(I32))
    with t.compile([(vdb.MetaTable.NE, 1, 1)], n) as cm:
        b = run_and_check(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, compiled_mask=cm, what="compiled mask")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the winner's best row for token 0 goes: the document is scored by its next row for that token
    plain = ix.search_batch_maxsim(toks, 10, t, 0, n_codes)
    win = int(plain[0][0, 0])
    members = np.nonzero(codes == win)[0]
    ok = np.ones(n, dtype=bool)
    ok[members[np.argmin(md.distances(metric, rows, toks[0][:1], codes == win)[0, members])]] = False
    mask, bits = dd.id_mask(ok)
    got = run_and_check(ix, t, metric, rows, codes, n_codes, toks, 10, ok=ok, id_mask=mask, mask_bits=bits, what="best row masked")
    at = np.nonzero(got[0][0] == win)[0]
    assert at.size == 0 or got[1][0, at[0]] > plain[1][0, 0]


def test_removed_rows_and_after_compact(vdb):
    rows, codes, n_codes, ix, t = setup(vdb, md.DOT, 1000, 64, "mixed")
    toks = md.tokens(64, (1, 9, 32))
    live = np.ones(1000, dtype=bool)
    for i in list(range(0, 1000, 7)) + list(range(60, 70)) + list(range(310, 590)):   # one document goes entirely, the long run shrinks
        ix.remove(i)
        live[i] = False
    run_and_check(ix, t, md.DOT, rows, codes, n_codes, toks, 20, ok=live, what="removed")
    ix.compact()
    run_and_check(ix, t, md.DOT, rows, codes, n_codes, toks, 20, ok=live, what="compacted")


def test_split_store_converts_back(vdb):
    n, dim, metric = 66000, 64, md.EUCLID
    rows, codes = md.rows(n, dim), (np.arange(n) // 16).astype(I32)
    ix, t = make_index(vdb, metric, rows), make_table(vdb, codes)
    ix.set_split(2)
    ix.search_batch_arrays(rows[:2], 5)
    assert ix.layout()[0] == SPLIT
    run_and_check(ix, t, metric, rows, codes, n // 16 + 1, md.tokens(dim, (3, 32)), 10, what="split")
    assert ix.layout()[0] == LAYOUT_F32                                        # (an f32 reader converts the store back)


def test_exact_duplicate_documents_tie_to_the_lower_code(vdb):
    rows = md.rows(300, 20).copy()
    rows[208:224] = rows[96:112]                                               # document 13 is document 6 again
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 300, 20, "adjacent", rows)
    got = run_and_check(ix, t, md.EUCLID, rows, codes, n_codes, [np.ascontiguousarray(rows[96:99] + F32(0.001), dtype=F32)], 5)
    assert got[0][0, :2].tolist() == [6, 13] and got[1][0, 0].view(np.uint32) == got[1][0, 1].view(np.uint32)


def test_chunk_boundary_five_queries_and_a_cap_for_two(vdb):
    rows, codes, n_codes, ix, t = setup(vdb, md.COSINE, 257, 33, "mixed")
    toks = md.tokens(33, (32, 1, 8, 17, 5))
    whole = run_and_check(ix, t, md.COSINE, rows, codes, n_codes, toks, 9)
    ix.debug_set_maxsim_table_cap(2 * n_codes * (32 * 4 + 8))
    capped = run_and_check(ix, t, md.COSINE, rows, codes, n_codes, toks, 9, chunks=3, what="capped")
    assert all(np.array_equal(x, y) for x, y in zip(whole, capped))


def test_an_inf_distance_inside_a_minimum_and_an_inf_score(vdb):
    rows = md.rows(257, 20).copy()
    rows[16, 3] = F32(3e38)                                                    # document 1: one row at +inf, fifteen finite
    rows[32:48, 5] = F32(-3e38)                                                # document 2: every row at +inf
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 257, 20, "adjacent", rows)
    got = run_and_check(ix, t, md.EUCLID, rows, codes, n_codes, md.tokens(20, (1, 9)), 1024)
    for b in range(2):
        c = int(got[2][b])
        assert got[0][b, c - 1] == 2 and np.isposinf(got[1][b, c - 1]) and np.isfinite(got[1][b, :c - 1]).all()


@pytest.mark.parametrize("metric", md.METRICS)
def test_one_token_is_search_batch_distinct_under_exists(vdb, metric):
    rows, codes, n_codes, ix, t = setup(vdb, metric, 1000, 33, "mixed")
    toks = md.tokens(33, (1, 1, 1))
    got = ix.search_batch_maxsim(toks, 40, t, 0, n_codes)
    with t.compile([(vdb.MetaTable.EXISTS, 0, 0)], 1000) as cm:
        _, dists, dcodes, counts = ix.search_batch_distinct(np.concatenate(toks), 40, t, 0, compiled_mask=cm)
    assert np.array_equal(got[2], counts) and np.array_equal(got[0], dcodes) and np.array_equal(got[1].view(np.uint32), dists.view(np.uint32))


def raw(vdb, ix, t, offsets, n_codes, dim=20, k=4, kstride=4, slot=0):
    off, tok = np.asarray(offsets, dtype=np.uintp), np.ones((64, dim), dtype=F32)
    oc, os_, cnt = np.full(4 * kstride, 12345, dtype=I32), np.zeros(4 * kstride, dtype=F32), np.full(4, 12345, dtype=np.uintp)
    szp, fp = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_float)
    rc = vdb._ffi.lib().vdb_flat_search_batch_maxsim(ix._h, tok.ctypes.data_as(fp), off.ctypes.data_as(szp), off.size - 1, dim, None, k,
                                                    t._t if t is not None else None, slot, n_codes, None, 0, kstride,
                                                    oc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), os_.ctypes.data_as(fp), cnt.ctypes.data_as(szp))
    return rc, vdb._ffi.last_error()[0], oc, cnt


def test_every_refusal_in_order_and_nothing_written(vdb):
    E = vdb._ffi.ERR_INVALID_ARGUMENT
    rows, codes, n_codes, ix, t = setup(vdb, md.EUCLID, 257, 20, "mixed")
    # (1) answered before every check: an empty index, k = 0
    for h, k in ((vdb.GpuFlatIndex(vdb.DistanceMetric(0), keep_host_copy=False), 4), (ix, 0)):
        rc, _, oc, cnt = raw(vdb, h, None, [5, 2], 0, k=k)
        assert rc == 0 and cnt[0] == 0 and (oc == 12345).all()
    # (2) .. (7): each call is wrong in its own step and in every later one
    sharded = make_index(vdb, md.EUCLID, rows, devices=[0, 0])
    for h, args, word in ((ix, dict(offsets=[0, 3, 2], n_codes=0, t=None, dim=7), "offsets decrease"),
                          (ix, dict(offsets=[0, 3, 3], n_codes=0, t=None, dim=7), "0 tokens"),
                          (ix, dict(offsets=[0, 33], n_codes=0, t=None, dim=7), "33 tokens"),
                          (ix, dict(offsets=[0, 3], n_codes=0, t=None, dim=7), "n_codes"),
                          (ix, dict(offsets=[0, 3], n_codes=n_codes, t=None, dim=7), "table"),
                          (ix, dict(offsets=[0, 3], n_codes=n_codes, t=t, slot=3, dim=7), "slot"),
                          (ix, dict(offsets=[0, 3], n_codes=n_codes, t=t, k=1025, kstride=1025, dim=7), "at most 1024"),
                          (sharded, dict(offsets=[0, 3], n_codes=n_codes, t=t, dim=7), "sharded"),
                          (ix, dict(offsets=[0, 3], n_codes=n_codes, t=t, dim=7), "imension")):
        rc, msg, oc, cnt = raw(vdb, h, args.pop("t"), **args)
        assert rc != 0 and (rc == E or word == "imension") and word in msg, (word, rc, msg)
        assert (oc == 12345).all() and (cnt == 12345).all(), word
    sharded.add(257, vdb.Vector(rows[0]))                                      # the sharded refusal comes before the flush of a staged row
    assert raw(vdb, sharded, t, [0, 3], n_codes)[0] == E
    with pytest.raises(vdb.VectorDbError):
        ix.search_batch_maxsim(md.tokens(20, (2,)), 4, t, 0, 100)              # the column holds codes up to 436


def test_nan_from_a_row_nan_from_the_sum_and_cosine_zero_norms(vdb):
    n, dim = 257, 20
    rows = md.rows(n, dim).copy()
    rows[40, 0] = np.inf                                                       # inf * 0 under Dot
    rows, codes, n_codes, ix, t = setup(vdb, md.DOT, n, dim, "adjacent", rows)
    tok = md.tokens(dim, (3,))[0].copy()
    ix.search_batch_maxsim([tok], 5, t, 0, n_codes)                            # inf * x: an infinite distance, no error
    tok[1, 0] = 0
    with pytest.raises(vdb.NanDistance):
        ix.search_batch_maxsim([tok], 5, t, 0, n_codes)
    with pytest.raises(md.NanDistance):
        md.expected(md.DOT, rows, codes, [tok], 5)
    # +inf and -inf meet in the sum: document 32 is one row whose dot products with the two tokens overflow to either side
    rows = np.zeros((48, dim), dtype=F32)
    rows[:, 1], rows[32, 0] = 1, F32(3e38)
    tok = np.zeros((2, dim), dtype=F32)
    tok[0, 0], tok[1, 0] = F32(3e38), F32(-3e38)
    ix, t1 = make_index(vdb, md.DOT, rows), make_table(vdb, np.arange(48))
    got = ix.search_batch_maxsim([tok[:1]], 5, t1, 0, 48)
    assert got[0][0, 0] == 32 and np.isneginf(got[1][0, 0])                    # one side alone is an ordinary -inf score
    with pytest.raises(vdb.NanDistance):
        ix.search_batch_maxsim([tok], 5, t1, 0, 48)
    # Cosine: a zero-norm token, a live zero-norm row
    ix = make_index(vdb, md.COSINE, md.rows(n, dim))
    tok = md.tokens(dim, (3,))[0].copy()
    tok[2] = 0
    with pytest.raises(vdb.InvalidVector):
        ix.search_batch_maxsim([tok], 5, t, 0, n_codes)
    ix.add(n, vdb.Vector(np.zeros(dim, dtype=F32)))
    with pytest.raises(vdb.InvalidVector):
        ix.search_batch_maxsim(md.tokens(dim, (3,)), 5, t, 0, n_codes)


@pytest.mark.parametrize("device_filter", [True, False])
def test_store_search_late_interaction_on_both_filter_paths(vdb, device_filter):
    n, dim, k = 600, 20, 8
    rows = md.rows(n, dim)
    doc = np.array([-1 if i % 13 == 0 else (i * 7) % 40 for i in range(n)], dtype=I32)
    lang = [("en", "de", "fr")[i % 3] for i in range(n)]
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    st.set_device_filter(device_filter)
    for i in range(n):
        meta = dict({"lang": lang[i]}, **({"doc": f"doc-{doc[i]}"} if doc[i] >= 0 else {}))
        st.insert_with_metadata(f"item-{i}", vdb.Vector(rows[i]), vdb.Metadata(meta))
    toks = md.tokens(dim, (5, 32))
    queries = [[vdb.Vector(v) for v in block] for block in toks]
    for flt, ok in ((None, None), (vdb.MetadataFilter.Eq("lang", "de"), np.array([x == "de" for x in lang]))):
        got = st.search_late_interaction_batch(queries, k, "doc", flt)
        for b, (wc, ws) in enumerate(md.expected(md.EUCLID, rows, doc, toks, k, ok=ok)):
            assert [v for v, _ in got[b]] == [f"doc-{c}" for c in wc]
            assert np.array_equal(np.array([s for _, s in got[b]], dtype=F32).view(np.uint32), ws.view(np.uint32))
        assert st.search_late_interaction(queries[1], k, "doc", flt) == got[1]
    assert st.search_late_interaction(queries[0], k, "nobody-has-this") == []

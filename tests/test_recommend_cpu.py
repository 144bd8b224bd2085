"""CPU proofs behind tests/test_gpu_recommend.py: the library exports the recommend entry points, and the data of
tests/recommend_data.py makes a wrong kernel VISIBLE -- on the requests the GPU tests use, the left fold differs from the reverse
fold, the multiply by the f32 reciprocal differs from the division, a leading -0.0 keeps its sign, and under Dot both outcomes of
the strike occur."""
import os
import re

import numpy as np
import pytest

import oracle
import by_id_data as bd
import recommend_data as rd
from conftest import load_package

F32, U64 = np.float32, np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vdb_flat_recommend_batch", "vdb_flat_recommend_batch_filtered", "vdb_flat_recommend_stats")


def test_library_exports_and_ffi_declares_the_three_symbols():
    vdb = load_package()
    vdb.build()
    L = vdb._ffi.lib()
    header = open(os.path.join(ROOT, "include", "vdb_flat.h")).read()
    for name in NAMES:
        assert name in vdb._ffi.SYMBOLS
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert len(L.vdb_flat_recommend_batch.argtypes) == 13 and len(L.vdb_flat_recommend_batch_filtered.argtypes) == 12
    assert re.search(r"#define VDB_RECOMMEND_MAX_EXAMPLES %d\b" % rd.MAX_EXAMPLES, header)
    assert L.vdb_abi_version() == 1
    for cls, names in ((vdb.GpuFlatIndex, ("recommend_batch", "recommend_stats")), (vdb.VectorStore, ("recommend", "recommend_batch"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def reverse_fold(rows, pos, neg):
    return rd.fold(rows, list(pos)[::-1], list(neg)[::-1])


def divided_fold(rows, pos, neg):
    def avg(lst):
        s = rows[lst[0]].astype(F32, copy=True)
        for r in lst[1:]:
            s = s + rows[r]
        return s if len(lst) == 1 else s / F32(len(lst))
    ap = avg(list(pos))
    return ap if not neg else ap + (ap - avg(list(neg)))


@pytest.mark.parametrize("dim", [33, 64, 1100])
def test_order_and_multiply_are_observable_on_the_fold_family(dim):
    rows = rd.fold_rows(dim)
    reqs = rd.fold_requests()
    order = mult = 0
    for p, n in reqs:
        q = rd.fold(rows, p, n)
        assert q.dtype == F32 and q.shape == (dim,)
        r, d = reverse_fold(rows, p, n), divided_fold(rows, p, n)
        if len(p) >= 3 or len(n) >= 3:
            assert (q.view(np.uint32) != r.view(np.uint32)).any(), (p, n)        # every request with three or more on a side
            order += 1
        else:
            assert np.array_equal(q.view(np.uint32), r.view(np.uint32))          # (two addends commute)
        if any(len(s) not in (0, 1, 2, 4, 64) for s in (p, n)):                  # (a power of two divides exactly)
            mult += int((q.view(np.uint32) != d.view(np.uint32)).any())
    print(f"dim {dim}: the reverse fold differs for {order} requests, the division for {mult}")
    assert order >= 6 and mult >= 4
    # ... and it reaches the answer: some request's distances change under the reverse fold
    qs = rd.queries(rows, reqs)
    qr = np.stack([reverse_fold(rows, p, n) for p, n in reqs])
    a = oracle.search_batch(rd.EUCLID, rows, qs, rd.K + 64)
    b = oracle.search_batch(rd.EUCLID, rows, qr, rd.K + 64)
    assert any(not np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(a, b))


def test_a_leading_negative_zero_keeps_its_sign():
    rows = rd.fold_rows(33)
    reqs = rd.fold_requests()
    assert reqs[0] == ((0,), ()) and reqs[2] == ((0, 1), ())
    assert np.signbit(rows[0, 0]) and rows[0, 0] == 0 and np.signbit(rows[1, 0])
    assert np.signbit(rd.fold(rows, *reqs[0])[0])                                # np = 1: the stored row itself
    assert np.signbit(rd.fold(rows, *reqs[2])[0])                                # -0 + -0 = -0, times 0.5
    assert not np.signbit((F32(0) + rows[0, 0] + rows[1, 0]))                    # a fold started from 0 loses it
    assert np.array_equal(rd.fold(rows, (17,), ()).view(np.uint32), rows[17].view(np.uint32))


def test_scaled_family_has_both_strike_outcomes_under_dot():
    rows = bd.scaled()
    reqs = rd.scaled_requests()
    res = oracle.search_batch(rd.DOT, rows, rd.queries(rows, reqs), [rd.K + len(p) + len(n) for p, n in reqs])
    found = absent = 0
    for (oi, _), (p, n) in zip(res, reqs):
        hit = np.isin(np.asarray(p + n, dtype=U64), oi)
        found += int(hit.sum())
        absent += int((~hit).sum())
    print(f"Dot, k = {rd.K}: {found} examples are among their request's k + m nearest, {absent} are not")
    assert found >= len(reqs) // 2 and absent >= len(reqs) // 2
    want = rd.expected_cached("scaled24", rd.DOT, rows, reqs, rd.K)
    assert all(len(oi) == rd.K and not np.isin(oi, np.asarray(p + n, dtype=U64)).any() for (oi, _), (p, n) in zip(want, reqs))
    assert rd.stats(rd.DOT, rows, reqs, rd.K, bd.N)[:2] == [len(reqs), sum(len(p) + len(n) for p, n in reqs)]


@pytest.mark.parametrize("metric", rd.METRICS)
def test_striking_m_from_k_plus_m_equals_the_search_without_the_examples(metric):
    """The identity the feature rests on: top k of (eligible rows without the examples) = top k + m of (eligible rows), minus the
    examples, cut to k -- also when an id is listed twice (m counts it twice, the set once)."""
    rows = rd.fold_rows(64)
    reqs = rd.fold_requests()
    for (p, n), (oi, od) in zip(reqs, rd.expected(metric, rows, reqs, rd.K)):
        live = np.ones(len(rows), dtype=np.uint8)
        live[list(p + n)] = 0
        wi, wd = oracle.flat_search(metric, rows, rd.fold(rows, p, n), rd.K, live=live)
        assert np.array_equal(oi, wi) and np.array_equal(od.view(np.uint32), wd.view(np.uint32)), (p, n)


def test_one_positive_is_search_by_id():
    rows = bd.scaled()
    sel = bd.spaced(bd.N, 12)
    for metric in rd.METRICS:
        a = rd.expected(metric, rows, [((int(r),), ()) for r in sel], rd.K)
        b = bd.expected(metric, rows, sel, rd.K)
        for (ai, ad), (bi, bdist, _, _) in zip(a, b):
            assert np.array_equal(ai, bi) and np.array_equal(ad.view(np.uint32), bdist.view(np.uint32))


def test_the_straddling_request_has_examples_on_both_sides_of_the_chunk_edge():
    rows, ids = bd.triplicates()
    pos, neg = rd.tri_straddle()
    assert len(pos) == rd.TRI_M and not neg
    (oi, _), = oracle.search_batch(rd.EUCLID, rows, rd.queries(rows, [(pos, neg)]), rd.TRI_K + rd.TRI_M, ids=ids)
    at = np.nonzero(np.isin(oi, ids[list(pos)]))[0]
    print("examples at list positions", at.tolist())
    assert len(oi) == 270 and (at < 255).sum() >= 2 and (at >= 256).sum() >= 1
    (si, sd), = rd.expected(rd.EUCLID, rows, [(pos, neg)], rd.TRI_K, ids=ids)
    assert len(si) == rd.TRI_K


def test_strike_counts_at_the_edges():
    """count = min(k, eligible rows - eligible examples)"""
    rows = bd.scaled(64, 8)
    req = [((3, 7, 9), (11,))]
    for k, n_want in ((0, 0), (1, 1), (60, 60), (61, 60), (64, 60), (500, 60)):
        (oi, od), = rd.expected(rd.EUCLID, rows, req, k)
        assert len(oi) == n_want, (k, len(oi))
    live = np.ones(64, dtype=np.uint8)
    live[[3, 11]] = 0                                                          # two examples are not eligible: still examples
    (oi, od), = rd.expected(rd.EUCLID, rows, req, 500, live=live)
    assert len(oi) == 60 and not np.isin(oi, [3, 7, 9, 11]).any()
    (oi, od), = rd.expected(rd.EUCLID, bd.scaled(4, 8), [((0, 1), (2, 3))], 5)
    assert len(oi) == 0                                                        # len <= m: nobody is left

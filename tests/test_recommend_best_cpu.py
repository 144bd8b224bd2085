"""CPU proofs behind tests/test_gpu_recommend_best.py (vdb_flat_recommend_best_batch): the library exports the
entry points; the restatement of the list route -- frontier, settled entries, capacity, walk, veto, escalation -- gives the
definition's answer on every family, metric and route (the proof that the frontier rule is sound); the three veto families end at
list stage 0, list stage 1 and the exact scan; the two-blob answer is one the average-vector recommend cannot give; and the
argument checks refuse through the library before anything touches a handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import recommend_data as rd
import recommend_best_data as rb
from conftest import load_package

F32, U64 = np.float32, np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vdb_flat_recommend_best_batch", "vdb_flat_recommend_best_batch_filtered", "vdb_flat_recommend_best_stats",
         "vdb_flat_debug_set_recommend_best_route")


def test_library_exports_and_ffi_declares_the_symbols():
    vdb = load_package()
    vdb.build()
    L = vdb._ffi.lib()
    header = open(os.path.join(ROOT, "include", "vdb_flat.h")).read()
    for name in NAMES:
        assert name in vdb._ffi.SYMBOLS
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "vdb_flat_recommend_best_depth" in vdb._ffi.SYMBOLS and re.search(r"\bsize_t vdb_flat_recommend_best_depth\(", header)
    assert len(L.vdb_flat_recommend_best_batch.argtypes) == 14 and len(L.vdb_flat_recommend_best_batch_filtered.argtypes) == 13
    assert re.search(r"#define VDB_RECOMMEND_BEST_MAX_K %d\b" % rb.MAX_K, header)
    assert L.vdb_abi_version() == 1
    for cls, names in ((vdb.GpuFlatIndex, ("recommend_best_batch", "recommend_best_stats", "debug_set_recommend_best_route")),
                       (vdb.VectorStore, ("recommend_best", "recommend_best_batch"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_depth_values():
    L = load_package()._ffi.lib()
    d = L.vdb_flat_recommend_best_depth
    for k, m, n in ((10, 1, 600), (10, 12, 600), (1, 1, 20), (1, 1, 40), (10, 64, 600), (500, 64, 5000), (600, 64, 600), (10, 3, 66000),
                    (2 ** 64 - 1, 64, 3000), (10, 2, 0)):
        for stage in (0, 1, 2, -1):
            assert d(k, m, n, stage) == rb.depth(k, m, n, stage), (k, m, n, stage)
    assert d(10, 1, 600, 0) == 32 and d(10, 12, 600, 0) == 44 and d(500, 64, 5000, 0) == 1024 and d(10, 64, 600, 1) == 600
    assert d(1, 1, 20, 0) == 20 and d(10, 3, 66000, 1) == 1024 and d(10, 3, 66000, 2) == 0


@pytest.mark.parametrize("metric", rb.METRICS)
@pytest.mark.parametrize("name", sorted(rb.FAMILIES))
def test_lists_restatement_equals_the_definition(name, metric):
    rows, ids, reqs = rb.FAMILIES[name]()
    want = rb.definition(name, metric, rows, reqs, rb.K, ids=ids)
    for route in (rb.AUTO, rb.LISTS, rb.SCAN):
        got, stages, st = rb.lists_route(name, metric, rows, reqs, rb.K, ids=ids, route=route)
        rb.same(got, want, (name, metric, route))
        assert st[2] + st[3] + st[4] == len(reqs) and st[0] == len(reqs)
        if route == rb.SCAN:
            assert stages == [rb.STAGE_SCAN] * len(reqs) and st[6] == 0
    for (oi, dp, dn), (p, n) in zip(want, reqs):
        assert not np.isin(oi, (np.arange(len(rows), dtype=U64) if ids is None else ids)[list(p) + list(n)]).any()
        assert (dp < dn).all() and (np.diff(rb.ordered(dp).astype(np.int64)) >= 0).all()
        assert len(oi) == 0 or np.isinf(dn).all() == (len(n) == 0)               # (a request may keep nothing at all)


def test_restatement_under_a_mask_removed_rows_and_per_request_k():
    rows, ids, reqs = rb.fold_family(33)
    rng = np.random.default_rng(5)
    live = np.ones(len(rows), dtype=np.uint8)
    dead = [r for r in rng.choice(len(rows), 60, replace=False) if not any(r in p + n for p, n in reqs)]
    live[dead] = 0
    mask = (rng.random(len(rows)) < 0.5).astype(np.uint8)
    ks = [1 + (7 * b) % 23 for b in range(len(reqs))]
    for metric in rb.METRICS:
        want = rb.definition("fold33-lm", metric, rows, reqs, ks, live=live, mask=mask)
        got, _, _ = rb.lists_route("fold33-lm", metric, rows, reqs, ks, live=live, mask=mask, route=rb.LISTS)
        rb.same(got, want, metric)
        for (oi, _, _), kb in zip(want, ks):
            assert len(oi) <= kb and live[oi.astype(np.int64)].all() and mask[oi.astype(np.int64)].all()


@pytest.mark.parametrize("metric", (rb.EUCLID, rb.COSINE))
def test_the_veto_families_end_at_stage_0_stage_1_and_the_scan(metric):
    for name, stage in (("trap", 0), ("veto100", 1), ("veto1500", rb.STAGE_SCAN)):
        rows, ids, reqs = rb.FAMILIES[name]()
        want, stages, st = rb.expected(name, metric, rows, reqs, rb.K, ids=ids)
        print(name, metric, "stages", stages, "stats", st)
        assert list(stages) == [stage], (name, metric, stages)
        assert len(want[0][0]) == rb.K
    # the density trap vetoes nothing among its answer's neighbourhood: the answer is the no-negative answer
    rows, ids, reqs = rb.trap()
    plain = rb.definition("trap-plain", metric, rows, [(reqs[0][0], ())], rb.K)
    assert np.array_equal(plain[0][0], rb.expected("trap", metric, rows, reqs, rb.K)[0][0][0])
    # veto-100: about a hundred of the nearest rows are vetoed before the first kept one
    rows, ids, reqs = rb.veto100()
    first = int(rb.expected("veto100", metric, rows, reqs, rb.K)[0][0][0][0])
    oi = rb.ranking("veto100", metric, rows, reqs[0][0][0], None, None)[0]
    at = int(np.nonzero(oi == first)[0][0])
    print("veto100", metric, "first kept row at list position", at)
    assert 80 <= at <= 200
    rows, ids, reqs = rb.veto1500()
    first = int(rb.expected("veto1500", metric, rows, reqs, rb.K)[0][0][0][0])
    oi = rb.ranking("veto1500", metric, rows, reqs[0][0][0], None, None)[0]
    assert int(np.nonzero(oi == first)[0][0]) > 1024


def test_two_blobs_are_both_found_and_the_average_finds_neither():
    rows, ids, reqs = rb.two_blob()
    (oi, dp, dn), _ = rb.definition("blob", rb.EUCLID, rows, reqs, rb.K)
    a = (oi < rb.BLOB_EACH).sum()
    b = ((oi >= rb.BLOB_EACH) & (oi < 2 * rb.BLOB_EACH)).sum()
    assert a >= 2 and b >= 2 and a + b == rb.K
    side = (oi >= rb.BLOB_EACH).astype(int)
    assert (np.diff(side) != 0).sum() >= 2                                     # interleaved, not one blob after the other
    (ai, _), = rd.expected(rb.EUCLID, rows, [reqs[0]], rb.K)
    mid = (ai >= 2 * rb.BLOB_EACH) & (ai < 2 * rb.BLOB_EACH + rb.BLOB_MID)
    assert mid.all() and not np.isin(ai, oi).any()


def test_tri_family_has_a_tie_at_the_frontier_and_a_request_that_keeps_nothing():
    rows, ids, reqs = rb.tri()
    want, stages, st = rb.expected("tri", rb.EUCLID, rows, reqs, rb.K, ids=ids)
    oi, od, _ = rb.ranking("tri", rb.EUCLID, rows, reqs[0][0][0], ids, None)
    D0 = st[5]
    assert od[D0 - 1] == od[D0] or od[D0 - 1] == od[D0 - 2]                    # the list ends inside a run of equal distances
    assert len(want[1][0]) == 0 and stages[1] == rb.STAGE_SCAN                 # dp == dn everywhere: all vetoed, proved by the scan only
    assert len(want[0][0]) == rb.K and len(want[2][0]) == rb.K


def test_inf_family():
    rows, ids, reqs = rb.inf_family()
    want = rb.definition("inf", rb.EUCLID, rows, reqs, 1000)
    got, stages, _ = rb.lists_route("inf", rb.EUCLID, rows, reqs, 1000, route=rb.LISTS)
    rb.same(got, want)
    # without negatives the +inf rows close the answer with dp = +inf ...
    oi, dp, dn = want[1]
    assert np.isinf(dp[-len(rb.INF_ROWS):]).all() and set(oi[-len(rb.INF_ROWS):].tolist()) == set(rb.INF_ROWS)
    assert np.isfinite(dp[:-len(rb.INF_ROWS)]).all() and len(oi) == rb.INF_N - 1
    # ... with a negative they are vetoed: dp = +inf against d(n, x) = +inf is a tie
    oi, dp, dn = want[0]
    assert len(oi) > rb.K and not np.isin(oi, rb.INF_ROWS).any() and np.isfinite(dp).all()
    with pytest.raises(rb.NanDistance):
        rb.definition("inf", rb.EUCLID, rows, rb.inf_nan_request(), rb.K)


def test_argument_checks_refuse_before_any_handle_is_touched():
    vdb = load_package()
    L = vdb._ffi.lib()
    bad = vdb._ffi.ERR_INVALID_ARGUMENT
    szp, u32p = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32)

    def call(ids, offsets, n_pos, nq, filtered=False):
        ex = np.asarray(ids, dtype=U64)
        off = np.asarray(offsets, dtype=np.uintp)
        npos = np.asarray(n_pos, dtype=np.uint32)
        oi, od, on, oc = np.zeros(4, dtype=U64), np.zeros(4, dtype=F32), np.zeros(4, dtype=F32), np.zeros(4, dtype=np.uintp)
        head = (None, ex.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), off.ctypes.data_as(szp), npos.ctypes.data_as(u32p), nq, None, 1)
        tail = (1, oi.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), od.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                on.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), oc.ctypes.data_as(szp))
        if filtered:
            rc = L.vdb_flat_recommend_best_batch_filtered(*head, ctypes.c_void_p(16), *tail)   # (never dereferenced: the checks come first)
        else:
            rc = L.vdb_flat_recommend_best_batch(*head, None, 0, *tail)
        return rc, vdb._ffi.last_error()[0]

    # the handle is NULL throughout: every refusal below names the ARGUMENT, so it came before the handle was looked at
    for filtered in (False, True):
        rc, msg = call([1, 2], [1, 2], [1], 1, filtered)
        assert rc == bad and "offsets[0]" in msg, msg
        rc, msg = call([1, 2], [0, 2, 1], [1, 1], 2, filtered)
        assert rc == bad and "decrease" in msg, msg
        rc, msg = call([1, 2], [0, 2], [0], 1, filtered)
        assert rc == bad and "no positive" in msg, msg                         # np = 0 is out of scope
        rc, msg = call([1, 2], [0, 2], [3], 1, filtered)
        assert rc == bad and "positives among" in msg, msg
        rc, msg = call(list(range(65)), [0, 65], [1], 1, filtered)
        assert rc == bad and "more than 64" in msg, msg
        rc, msg = call([1, 2], [0, 2], [1], 1, filtered)
        assert rc == bad and "null argument" in msg, msg                       # everything else is fine: now the handle
    out = (ctypes.c_uint64 * 8)()
    assert L.vdb_flat_recommend_best_stats(None, out) == bad
    assert L.vdb_flat_debug_set_recommend_best_route(None, 0) == bad
    oc = np.zeros(1, dtype=np.uintp)
    assert L.vdb_flat_recommend_best_batch_filtered(None, None, None, None, 0, None, 1, None, 1, None, None, None, oc.ctypes.data_as(szp)) == bad

"""What tests/test_gpu_per_group.py assumes, shown on the CPU: the host plan of vdb_flat_search_batch_per_group
against numpy.unique, and the properties of the test families -- that no plain search reaches the members the scattered family
expects, that the separated families put pairs on both routes once the scan cap is lowered, and what the tied rows answer."""
import ctypes
import os

import numpy as np
import pytest

import distinct_data as dd
import per_group_data as pg
import range_data as rd
from conftest import ROOT, load_package


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def check_plan(vdb, codes, kept, ks=None):
    got = vdb.GpuFlatIndex.debug_per_group_plan(codes, kept, ks)
    want = pg.plan(codes, kept, ks)
    assert got is not None
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1])
    return got


def test_plan_equals_numpy_unique_on_random_input(vdb):
    rng = np.random.default_rng(20273)
    for nq, kmax, hi in ((1, 1, 3), (7, 10, 12), (64, 33, 5000), (256, 10, 40), (3, 1024, 2 ** 31 - 1)):
        codes = rng.integers(-1, hi, (nq, kmax)).astype(np.int32)
        codes[rng.random((nq, kmax)) < 0.2] = -1
        kept = rng.integers(0, kmax + 3, nq).astype(np.uint32)                 # (a count above the stride is clamped)
        wanted, index = check_plan(vdb, codes, kept)
        assert (np.diff(wanted) > 0).all() and (wanted >= 0).all()
        ks = rng.integers(0, kmax + 1, nq)
        check_plan(vdb, codes, kept, ks)
        # the prefix property: the plan for ks counts a subset of the plan for max(ks)
        assert set(check_plan(vdb, codes, kept, ks)[0].tolist()) <= set(wanted.tolist())


def test_plan_on_degenerate_input(vdb):
    none = np.full((5, 4), -1, dtype=np.int32)
    wanted, index = check_plan(vdb, none, np.full(5, 4, dtype=np.uint32))
    assert wanted.size == 0 and (index == pg.NONE).all()
    one = np.full((5, 4), 77, dtype=np.int32)
    wanted, index = check_plan(vdb, one, np.full(5, 4, dtype=np.uint32))
    assert wanted.tolist() == [77] and (index == 0).all()
    wanted, index = check_plan(vdb, one, np.zeros(5, dtype=np.uint32))          # kept = 0: nothing is counted
    assert wanted.size == 0 and (index == pg.NONE).all()
    wanted, index = check_plan(vdb, one, np.full(5, 4, dtype=np.uint32), np.array([0, 1, 0, 4, 2]))
    assert wanted.tolist() == [77] and (index != pg.NONE).sum(axis=1).tolist() == [0, 1, 0, 4, 2]
    L = vdb._ffi.lib()
    bad = ctypes.c_size_t(-1).value
    assert L.vdb_flat_debug_per_group_plan(None, None, None, 3, 2, None, 0, None) == bad
    assert L.vdb_flat_debug_per_group_plan(None, None, None, 0, 0, None, 0, None) == 0
    assert vdb.GpuFlatIndex.debug_per_group_plan(np.zeros((1, 1025), dtype=np.int32), [1]) is None


def test_symbols_are_exported_and_bound(vdb):
    L = vdb._ffi.lib()
    for name in ("vdb_flat_search_batch_per_group", "vdb_flat_search_batch_per_group_filtered", "vdb_flat_per_group_stats",
                 "vdb_flat_debug_per_group_plan", "vdb_flat_debug_set_per_group_scan_cap"):
        assert name in vdb._ffi.SYMBOLS and hasattr(L, name)
    assert vdb.GpuFlatIndex.PER_GROUP_MAX_SIZE == pg.MAX_SIZE == 32
    header = open(os.path.join(ROOT, "include", "vdb_flat.h")).read()
    assert "#define VDB_PER_GROUP_MAX_SIZE 32" in header


@pytest.mark.parametrize("metric", pg.METRICS)
def test_scattered_members_lie_beyond_every_search(metric):
    """the deepest list any search returns holds 1024 rows: every query expects a member far beyond it"""
    rows, q, codes = pg.scattered()
    deepest = []
    for b in range(pg.SC_NQ):
        rank = rd.ranking(("per group scattered", b), metric, rows, q[b])
        groups = pg.expected(rank, codes, pg.SC_K, pg.SC_G)
        assert len(groups) == pg.SC_K and all(len(ids) == pg.SC_G for _, ids, _ in groups), b
        deepest.append(max(int(pos[-1]) + 1 for pos in pg.member_ranks(rank, codes, pg.SC_K, pg.SC_G)))
    print("deepest expected member per query, 1-based rank:", deepest)
    assert min(deepest) > dd.MAX_LIST, deepest


@pytest.mark.parametrize("metric", pg.METRICS)
@pytest.mark.parametrize("family", ["dominated", "giants"])
def test_separated_families_take_both_routes_under_the_low_cap(metric, family):
    rows, q, _ = rd.separated()
    codes = dd.dominated_codes() if family == "dominated" else dd.giant_codes()
    ranks = [rd.ranking(("sep", b), metric, rows, q[b]) for b in range(rd.NQ)]
    full = pg.routes(ranks, codes, dd.DOM_K, pg.SC_G)
    low = pg.routes(ranks, codes, dd.DOM_K, pg.SC_G, pg.LOW_CAP)
    print(family, "default cap:", full, "cap 1024:", low)
    assert full[2] == 0 and full[1] > 0                                        # 62k rows at most: every list fits the default cap
    assert low[1] > 0 and low[2] > 0                                           # the 3000-row cluster (and the background) do not fit 1024
    assert low[0] == full[0] and low[3] == full[3] and low[1] + low[2] == full[1]


@pytest.mark.parametrize("metric", pg.METRICS)
def test_tied_rows_are_members_in_id_order(metric):
    rows, q = rd.tied()
    codes = dd.tied_codes(True)
    rank = rd.ranking(("tied", 0), metric, rows, q[0])
    code, ids, dists = pg.expected(rank, codes, 5, 3)[0]
    assert code == 7 and ids.tolist() == sorted(rd.TIE_ROWS)[:3] and len(set(dists.view(np.uint32).tolist())) == 1
    code, ids, dists = pg.expected(rank, codes, 5, 8)[0]
    assert code == 7 and ids.tolist() == sorted(rd.TIE_ROWS)                   # five rows have the code: size 5

"""The plan of a grouped search (vdb_flat_debug_group_plan) and the argument checks of
vdb_flat_search_batch_grouped that need no device.  The plan is host arithmetic alone: no handle, no GPU."""
import ctypes

import numpy as np
import pytest

from conftest import load_package

NONE = 0xFFFFFFFF
SUPER, TILE, MAX_E = 256, 64, 131072


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def check_plan(vdb, group_of, elig):
    group_of = np.asarray(group_of, dtype=np.uint32)
    elig = np.asarray(elig, dtype=np.uint32)
    nq = group_of.size
    perm, tiles = vdb.GpuFlatIndex.debug_group_plan(group_of, elig)
    # perm is a permutation, and every group's queries are contiguous in it (the unfiltered ones are a "group" too)
    assert sorted(perm.tolist()) == list(range(nq))
    pg = group_of[perm] if nq else group_of
    seen = set()
    for i, g in enumerate(pg.tolist()):
        if i and g == pg[i - 1]:
            continue
        assert g not in seen, ("group not contiguous", g)
        seen.add(g)
    # inside a group the caller's order is kept
    for g in seen:
        pos = perm[pg == g]
        assert np.all(np.diff(pos.astype(np.int64)) > 0)
    scanned = lambda g: g != NONE and 0 < elig[g] <= MAX_E
    cover = {}
    for g, j0, q0, n in tiles.tolist():
        assert scanned(g), ("a tile for a group that is not scanned", g)
        assert 1 <= n <= TILE and j0 % TILE == 0 and j0 < elig[g]
        assert q0 + n <= nq and q0 // SUPER == (q0 + n - 1) // SUPER, "a tile spans two passes"
        assert np.all(pg[q0:q0 + n] == g), "a tile spans two groups"
        for q in range(q0, q0 + n):
            for j in range(j0, min(j0 + TILE, int(elig[g])), TILE):
                key = (q, j)
                assert key not in cover, ("pair block covered twice", key)
                cover[key] = 1
    # every (query, list position < E_g) of a scanned group lies in exactly one tile: all 64-blocks of all its queries are there
    want = 0
    for i, g in enumerate(pg.tolist()):
        if scanned(g):
            blocks = (int(elig[g]) + TILE - 1) // TILE
            want += blocks
            for jb in range(blocks):
                assert (i, jb * TILE) in cover, (i, jb)
    assert len(cover) == want
    # the scanned queries come first (so that pass p holds permuted queries [256 p, 256 p + 256))
    kinds = [0 if scanned(g) else 1 for g in pg.tolist()]
    assert kinds == sorted(kinds)
    return perm, tiles


def test_hand_made_plans(vdb):
    # interleaved groups, one empty, one beyond the capacity, unfiltered queries mixed in
    perm, tiles = check_plan(vdb, [2, 0, NONE, 2, 1, 0, 3, 2], [65, 0, 130, MAX_E + 1])
    assert perm.tolist() == [1, 5, 0, 3, 7, 4, 6, 2]
    assert tiles.tolist() == [[0, 0, 0, 2], [0, 64, 0, 2], [2, 0, 2, 3], [2, 64, 2, 3], [2, 128, 2, 3]]
    # nothing to scan at all
    for go, el in (([NONE] * 5, []), ([0, 0], [0]), ([0, NONE], [MAX_E + 1]), ([], [3, 4])):
        perm, tiles = check_plan(vdb, go, el)
        assert tiles.shape == (0, 4)
    # exactly at the capacity: scanned, 2048 list tiles
    _, tiles = check_plan(vdb, [0], [MAX_E])
    assert tiles.shape[0] == MAX_E // TILE
    # a bad group index
    assert vdb.GpuFlatIndex.debug_group_plan([1], [5]) is None
    assert vdb.GpuFlatIndex.debug_group_plan([NONE - 1], [5]) is None


@pytest.mark.parametrize("nq_of", [(1,), (63,), (64,), (65,), (300,), (200, 100), (255, 2, 255), (64, 64, 64, 64, 1)])
def test_query_counts_and_pass_edges(vdb, nq_of):
    go = np.concatenate([np.full(c, g, dtype=np.uint32) for g, c in enumerate(nq_of)])
    for E in (1, 63, 64, 65, 129):
        perm, tiles = check_plan(vdb, go, [E] * len(nq_of))
        assert np.array_equal(perm, np.arange(go.size))
    # a group cut by the pass boundary gets tiles on both sides
    if nq_of == (200, 100):
        _, tiles = check_plan(vdb, go, [1, 1])
        assert [t for t in tiles.tolist() if t[0] == 1] == [[1, 0, 200, 56], [1, 0, 256, 44]]


def test_random_plans(vdb):
    rng = np.random.default_rng(13)
    for trial in range(60):
        n_masks = int(rng.choice([1, 2, 7, 40]))
        nq = int(rng.integers(1, 700))
        elig = rng.choice([0, 1, 63, 64, 65, 129, 1000, MAX_E, MAX_E + 1, 4000000], size=n_masks).astype(np.uint32)
        go = rng.integers(0, n_masks, size=nq).astype(np.uint32)
        go[rng.random(nq) < 0.1] = NONE
        check_plan(vdb, go, elig)


def test_symbols_and_abi(vdb):
    L = vdb._ffi.lib()
    for name in ("vdb_flat_search_batch_grouped", "vdb_flat_search_batch_grouped_filtered", "vdb_flat_grouped_stats", "vdb_flat_debug_group_plan"):
        assert name in vdb._ffi.SYMBOLS and hasattr(L, name)
    assert L.vdb_abi_version() == 1
    assert vdb.GpuFlatIndex.GROUP_NONE == NONE


def test_argument_checks_without_a_device(vdb):
    L = vdb._ffi.lib()
    out = (ctypes.c_uint64 * 8)()
    assert L.vdb_flat_grouped_stats(None, out) == vdb._ffi.ERR_INVALID_ARGUMENT
    q = (ctypes.c_float * 4)()
    cnt = (ctypes.c_size_t * 1)()
    go = (ctypes.c_uint32 * 1)(NONE)
    # a null handle is refused before anything else, in both forms
    assert L.vdb_flat_search_batch_grouped(None, q, 1, 4, None, 1, None, 0, 0, go, 1, None, None, cnt) == vdb._ffi.ERR_INVALID_ARGUMENT
    assert L.vdb_flat_search_batch_grouped_filtered(None, q, 1, 4, None, 1, None, 0, go, 1, None, None, cnt) == vdb._ffi.ERR_INVALID_ARGUMENT
    assert "null" in vdb._ffi.last_error()[0]
    # the plan probe with null inputs: a bad call, not a crash
    assert L.vdb_flat_debug_group_plan(None, 3, None, 0, None, None, 0) == ctypes.c_size_t(-1).value
    assert L.vdb_flat_debug_group_plan(None, 0, None, 0, None, None, 0) == 0


def test_filter_keys_of_the_store(vdb):
    F = vdb.MetadataFilter
    key = vdb.VectorStore._filter_key
    a = F.And([F.Eq("t", "x"), F.Or([F.Ne("u", 3), F.Exists("v")])])
    b = F.And([F.Eq("t", "x"), F.Or([F.Ne("u", 3), F.Exists("v")])])
    assert key(a) == key(b) and hash(key(a)) == hash(key(b))
    for other in (F.And([F.Eq("t", "y"), F.Or([F.Ne("u", 3), F.Exists("v")])]), F.And([F.Or([F.Ne("u", 3), F.Exists("v")]), F.Eq("t", "x")]),
                  F.Or([F.Eq("t", "x"), F.Or([F.Ne("u", 3), F.Exists("v")])]), F.Eq("t", "x"), F.Ne("t", "x"), F.And([]), F.Or([]),
                  F.And([F.Eq("t", "x"), F.Or([F.Ne("u", 3.0), F.Exists("v")])])):
        assert key(other) != key(a)
    assert key(F.And([])) != key(F.Or([])) and key(F.And([F.And([])])) != key(F.And([]))

"""Stateful lifecycle tests on the GPU (tests/lifecycle.py; tests/test_lifecycle_cpu.py proves on the CPU that these schedules
catch stale state): long seeded schedules of interleaved mutations and reads through a GpuFlatIndex, through one sharded
handle and through VectorStore, every read compared bit for bit with the model -- ids, order, counts, distance bits, range
totals, group codes, the by-id struck / cut counters and the distinct stage counters, or the predicted error.

After each schedule the engine's own counters, accumulated over the run, must show that the routes were taken: the direct
path, dense scores of a small index, the fused f32 pass, the exact scan, the exact range scan, the sparse route, distinct stages A
and B, by-id struck and cut, compaction chunks moved directly and through the bounce buffer, a re-allocation with the shadow on.
The route of every plain search is also compared with the one its sizes are meant to take (lifecycle.predicted_route).

The bf16 screening tier, its sample copy and shadow rows, the screened range route and the dense range fallback start at
65 536 rows (32 768 survivors), above the 20 000 rows the twelve schedules are held to: three short schedules of 75 000 rows
(test_large_lifecycle) reach them and assert last_stats()["bf16_screen"], ["shadow_rows"], range_stats()[0] and [2].

What the counters can and cannot tell: the direct path and the exact scan both report exact_queries == nq and nothing else,
so "direct" against "exact" is told apart by the sizes only (the same rule predicted_route uses); what the route check does
prove is direct / exact against dense / fused / bf16.  grown_with_shadow is the adapter's own memory of set_shadow at a
capacity change; that the shadow is READ is the engine's shadow_rows flag, asserted in test_large_lifecycle.  On the sharded
runs every range read is refused, so more than 15 % of their reads expect an error (10-18 % refusals plus the episodes).

Twin equality: on a sample of plain searches the answer equals that of a fresh index bulk-loaded with the survivors, so a
failure says whether the model or the life before the read is at fault.

Grouped, recommend and numeric-filter reads (lifecycle.NEW_PINNED, NEW_STORE_PINNED): six index schedules of all nine read
kinds through a plain handle (grouped_stats [0]-[5] and recommend_stats [1]-[3] compared with the model read by read; the
grouped scan, the per-group fallback of k > 2048, unfiltered queries, folded examples, struck entries and numeric compiles
must all have been counted; twins with a fresh MetaTable on every fourth grouped / recommend read) and through a sharded
handle (every grouped read refused), three store schedules with numeric fields.  E_g > 131072 is out of reach at 20 000 rows.

MMR, per-group and recommend-by-best reads (lifecycle.TWELVE_PINNED, large-twelve, TWELVE_STORE_PINNED): six index schedules of
all twelve read kinds through a plain handle -- MMR's score bits, the groups' codes, sizes and members, the dn bits, and
mmr_stats [0]-[4], per_group_stats [1]-[6], recommend_best_stats [0]-[6] compared read by read; the counters must show MMR
pairs, member lists filled and giants searched, best answered at list stage 0, at stage 1 and by the exact scan; a twin on every
fourth read of each kind -- and through a sharded handle (all three refused, after the empty-index answer where the header puts
it first); one 75 000-row schedule whose inner searches run on the bf16 tier; two store schedules."""
import numpy as np
import pytest

import lifecycle as lc
from conftest import load_package

pytestmark = pytest.mark.gpu

NAMES = [p[0] for p in lc.PINNED]
LARGE_NAMES = [p[0] for p in lc.LARGE_PINNED]
STORE_NAMES = [p[0] for p in lc.STORE_PINNED]
NEW_NAMES = [p[0] for p in lc.NEW_PINNED]
NEW_STORE_NAMES = [p[0] for p in lc.NEW_STORE_PINNED]
TWELVE_NAMES = [p[0] for p in lc.TWELVE_PINNED]
TWELVE_STORE_NAMES = [p[0] for p in lc.TWELVE_STORE_PINNED]
_TRACES = {}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    return v


def trace_of(name):
    if name not in _TRACES:
        _TRACES[name] = lc.store_pinned(name) if name in STORE_NAMES + TWELVE_STORE_NAMES else lc.pinned(name)
    return _TRACES[name]


def same(a, b):
    return np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def life(vdb, name, devices=None):
    """one pinned schedule through an index adapter; returns the adapter's counters and what the model meant to reach"""
    t = trace_of(name)
    ad = lc.GpuIndexAdapter(vdb, t["metric"], devices=devices)
    meant, n_search, off_route = lc.Counter(), [0], []

    def on_read(step, op, model, args, got):
        if "error" in got:
            meant["error_" + got["error"][0]] += 1
            return
        if "stages" in got:
            meant["distinct_reads"] += 1
        want = lc.predicted_route(model, ad.settings, op, args)
        if want is not None and not ad.sharded:
            if ad.route != want:
                off_route.append((step, op, ad.route, want, ad.ix.last_stats()))
            meant["route_" + want] += 1
        if op[0] == "search":
            n_search[0] += 1
            if n_search[0] % 6 == 0:                                 # twin equality, on every sixth plain search
                rows, ids = model.survivors()
                twin = vdb.GpuFlatIndex(vdb.DistanceMetric(t["metric"]), keep_host_copy=False)
                twin.add_bulk(rows, ids=ids)
                assert same(ad.raw, twin.search_batch_arrays(args[0], args[1])), (name, step, op)
                meant["twins"] += 1
    try:
        lc.run(t, ad, expected=lc.slots(name, t), on_read=on_read)
    finally:
        ad.close()
    print(name, "sharded" if devices else "plain", dict(ad.seen), dict(meant))
    assert not off_route, off_route                                  # every predicted route was the one taken
    return ad.seen, meant


@pytest.mark.parametrize("name", NAMES)
def test_index_lifecycle(vdb, name):
    seen, meant = life(vdb, name)
    for route in ("direct", "dense", "fused", "exact"):
        assert meant["route_" + route] > 0 and seen["route_" + route] >= meant["route_" + route], (route, seen, meant)
    assert seen["range_exact"] > 0 and seen["sparse_route"] > 0, seen
    assert seen["distinct_a"] > 0 and seen["distinct_b"] > 0, seen
    assert seen["by_id_struck"] > 0 and seen["by_id_cut"] > 0, seen
    assert seen["chunks_direct"] > 0 and seen["chunks_bounce"] > 0 and seen["compactions"] >= 4, seen
    assert seen["grown"] >= 3 and seen["grown_with_shadow"] >= 1 and seen["shrunk"] >= 1, seen
    assert meant["twins"] >= 2, meant
    t = trace_of(name)
    if t["metric"] == lc.COSINE:
        assert meant["error_InvalidVector"] >= 2, meant
    if any(op[0] == "misfit" for op in t["ops"]):
        assert meant["error_DimensionMismatch"] >= 2, meant
    assert meant["error_VectorNotFound"] >= 1, meant


@pytest.mark.parametrize("name", LARGE_NAMES)
def test_large_lifecycle(vdb, name):
    """75 000 rows of d = 64: the bf16 screening tier with and without the shadow rows (the engine's own shadow_rows flag), with
    and without its sample copy, large k on it, the screened range route and the dense range fallback -- before and after a
    shrinking compaction refilled to the same row count.  Above the 20 000 rows the other schedules are held to: these routes
    start at 65 536 rows."""
    seen, meant = life(vdb, name)
    assert meant["route_bf16"] >= 10 and seen["route_bf16"] >= meant["route_bf16"], (seen, meant)
    assert seen["bf16_shadow_rows"] > 0 and seen["bf16_plain_rows"] > 0 and seen["bf16_large_k"] > 0, seen
    assert meant["route_fused"] > 0 and meant["route_exact"] > 0, meant          # set_screen(0); large k with set_large_k(0)
    assert seen["range_screened"] > 0 and seen["range_dense"] > 0 and seen["range_exact"] > 0, seen
    assert seen["grown_with_shadow"] >= 2 and seen["shrunk"] >= 1 and seen["compactions"] >= 3, seen
    assert seen["by_id_struck"] > 0 and seen["distinct_a"] > 0 and seen["sparse_route"] > 0 and meant["twins"] >= 2, (seen, meant)


@pytest.mark.parametrize("name", NAMES)
def test_sharded_lifecycle(vdb, name):
    seen, meant = life(vdb, name, devices=[0, 0, 0])
    t = trace_of(name)
    assert meant["error_Refused"] == sum(1 for op in t["ops"] if op[0] == "range") > 0, meant    # every range read, refused
    assert seen["range_exact"] == 0 and seen["sparse_route"] > 0, seen
    assert seen["distinct_a"] > 0 and seen["distinct_b"] > 0, seen
    assert seen["by_id_struck"] > 0 and seen["by_id_cut"] > 0, seen
    assert seen["compactions"] >= 4 and meant["twins"] >= 2, (seen, meant)


def life9(vdb, name, devices=None):
    """one schedule of the nine read kinds (lifecycle.NEW_PINNED) through an index adapter: every read against the model, the
    counters grouped_stats [0]-[5] and recommend_stats [1]-[3] with it (lifecycle.diff: "gstats", "rstats"); on a plain handle
    every fourth grouped and every fourth recommend read again on a twin -- a fresh index bulk-loaded with the survivors, a fresh
    MetaTable with the model's codes, presence bits and numbers.  Returns the adapter's counters, what was met, the model."""
    t = trace_of(name)
    ad = lc.GpuIndexAdapter(vdb, t["metric"], devices=devices)
    meant, nth = lc.Counter(), lc.Counter()

    def on_read(step, op, model, args, got):
        if "error" in got:
            meant[(op[0], got["error"][0])] += 1
            return
        meant[(op[0], "answered")] += 1
        meant["numeric_answered"] += lc.carries_numeric(op)
        if op[0] in ("grouped", "recommend") and not ad.sharded:
            nth[op[0]] += 1
            if nth[op[0]] % 4 == 0:
                twin = ad.twin(model)
                try:
                    again = getattr(twin, op[0])(*args)
                finally:
                    twin.close()
                what = lc.diff(got, again)
                assert what is None, (name, step, op, "the twin answers otherwise", what)
                meant["twins_" + op[0]] += 1
    try:
        model = lc.run(t, ad, expected=lc.slots(name, t), on_read=on_read)
    finally:
        ad.close()
    print(name, "sharded" if devices else "plain", dict(ad.seen), dict(meant), model.counts)
    return ad.seen, meant, model


@pytest.mark.parametrize("name", NEW_NAMES)
def test_index_lifecycle_nine(vdb, name):
    """grouped, recommend and numeric-masked reads in a long life of the index: doublings with the shadow on, a shrinking
    compaction that collides the row count, a reset to another dimension, auto-compaction inside the read, the zero-norm and
    misfit episodes, the LUT regrown twice between compiles, codes beyond the LUT.  E_g > 131072 is not reached (20 000 rows)."""
    seen, meant, model = life9(vdb, name)
    assert seen["grouped_scan"] > 0 and seen["grouped_fallback"] > 0 and seen["grouped_unfiltered"] > 0 and seen["grouped_tiles"] > 0, seen
    assert seen["recommend_examples"] > 0 and seen["recommend_struck"] > 0 and seen["numeric_compiles"] > 0, seen
    assert model.counts["regrows"] >= 2, model.counts
    assert meant["twins_grouped"] >= 1 and meant["twins_recommend"] >= 1, meant
    assert all(meant[(kind, "answered")] > 0 for kind in lc.READS9) and meant["numeric_answered"] > 0, meant
    t = trace_of(name)
    if t["metric"] == lc.COSINE:
        assert meant[("grouped", "InvalidVector")] >= 1 and meant[("recommend", "InvalidVector")] >= 1, meant
    if any(op[0] == "misfit" for op in t["ops"]):
        assert meant[("grouped", "DimensionMismatch")] >= 1 and meant[("recommend", "DimensionMismatch")] >= 1, meant
    assert meant[("recommend", "VectorNotFound")] >= 1, meant


@pytest.mark.parametrize("name", NEW_NAMES)
def test_sharded_lifecycle_nine(vdb, name):
    """the same schedules through one sharded handle: every grouped read is refused (as every range read is), recommend --
    examples gathered per shard -- and the numeric-masked reads are answered, recommend_stats as on the plain handle"""
    seen, meant, model = life9(vdb, name, devices=[0, 0, 0])
    t = trace_of(name)
    assert meant[("grouped", "Refused")] == sum(1 for op in t["ops"] if op[0] == "grouped") > 0, meant
    assert meant[("grouped", "answered")] == 0 and seen["grouped_scan"] + seen["grouped_fallback"] == 0, (seen, meant)
    assert meant[("recommend", "answered")] > 0 and meant[("numeric", "answered")] > 0 and meant["numeric_answered"] > 0, meant
    assert seen["recommend_examples"] > 0 and seen["recommend_struck"] > 0 and seen["numeric_compiles"] > 0, seen


def life12(vdb, name, devices=None, trace=None):
    """one schedule of the twelve read kinds (lifecycle.TWELVE_PINNED) through an index adapter: every read against the model --
    for the three composed reads the lists, MMR's score bits, the groups' codes, sizes and members, the dn bits, and
    mmr_stats [0]-[4], per_group_stats [1]-[6], recommend_best_stats [0]-[6] (lifecycle.diff).  On a plain handle every fourth
    read of each of the three kinds is made again on a twin -- a fresh index bulk-loaded with the survivors, a fresh MetaTable,
    the two debug switches as they stand -- and the two answers, counters included, are compared."""
    t = trace or trace_of(name)
    ad = lc.GpuIndexAdapter(vdb, t["metric"], devices=devices)
    meant, nth = lc.Counter(), lc.Counter()

    def on_read(step, op, model, args, got):
        if "error" in got:
            meant[(op[0], got["error"][0])] += 1
            return
        meant[(op[0], "answered")] += 1
        meant[(op[0], "rows")] += sum(len(l[0]) for l in got["lists"])
        if op[0] in lc.NEWER_READS and not ad.sharded:
            nth[op[0]] += 1
            if nth[op[0]] % 4 == 0:
                twin = ad.twin(model)
                try:
                    again = getattr(twin, op[0])(*args)
                finally:
                    twin.close()
                what = lc.diff(got, again)
                assert what is None, (name, step, op, "the twin answers otherwise", what)
                meant["twins_" + op[0]] += 1
    try:
        model = lc.run(t, ad, expected=lc.slots(name, t), on_read=on_read)
    finally:
        ad.close()
    print(name, "sharded" if devices else "plain", dict(ad.seen), dict(meant), model.counts)
    return ad.seen, meant, model


@pytest.mark.parametrize("name", TWELVE_NAMES)
def test_index_lifecycle_twelve(vdb, name):
    """MMR, per-group and recommend-by-best reads in a long life of the index: the row written last is a candidate behind every
    kind of write, compactions by hand and inside the read, doublings with both debug switches set, a reset to another
    dimension, the zero-norm and misfit episodes.  The engine's own counters must show the routes: MMR pairs, member lists
    filled and giants searched, best answered at list stage 0, at stage 1 and by the exact scan."""
    seen, meant, model = life12(vdb, name)
    assert seen["mmr_pairs"] > 0 and seen["mmr_candidates"] > 0, seen
    assert seen["per_group_filled"] > 0 and seen["per_group_giants"] > 0 and seen["per_group_listed"] > 0, seen
    assert seen["best_stage0"] > 0 and seen["best_stage1"] > 0 and seen["best_scan"] > 0 and seen["best_list_searches"] > 0, seen
    assert all(meant["twins_" + kind] >= 1 for kind in lc.NEWER_READS), meant
    assert all(meant[(kind, "answered")] > 0 and meant[(kind, "rows")] > 0 for kind in lc.READS12), meant
    t = trace_of(name)
    for kind in lc.NEWER_READS:
        if t["metric"] == lc.COSINE:
            assert meant[(kind, "InvalidVector")] >= 1, (kind, meant)
        if any(op[0] == "misfit" for op in t["ops"]):
            assert meant[(kind, "DimensionMismatch")] >= 1, (kind, meant)
    assert meant[("best", "VectorNotFound")] >= 1, meant


@pytest.mark.parametrize("name", TWELVE_NAMES)
def test_sharded_lifecycle_twelve(vdb, name):
    """the same schedules through one sharded handle: recommend by best refuses it before anything else, MMR and per group
    answer an empty index first and refuse it otherwise (these schedules never read an empty index: every read of the three is
    refused); the nine older kinds behave as before -- range and grouped refused, the others answered"""
    seen, meant, model = life12(vdb, name, devices=[0, 0, 0])
    t = trace_of(name)
    for kind in lc.NEWER_READS + ("range", "grouped"):
        assert meant[(kind, "Refused")] == sum(1 for op in t["ops"] if op[0] == kind) > 0, (kind, meant)
        assert meant[(kind, "answered")] == 0, (kind, meant)
    assert seen["mmr_pairs"] + seen["per_group_filled"] + seen["per_group_giants"] + seen["best_list_searches"] == 0, seen
    for kind in ("search", "masked", "sparse", "by_id", "distinct", "recommend", "numeric"):
        assert meant[(kind, "answered")] > 0, (kind, meant)


def test_large_lifecycle_twelve(vdb):
    """75 000 rows of d = 64: MMR's candidate search, the search by group inside per group and the list searches of recommend
    by best run on the bf16 screening tier -- the engine's own last_stats()["bf16_screen"] after every such read -- before
    and after a compaction and a shrinking compaction refilled to the same row count; one MMR read at m = 1024 with B = 1, whose
    depth leaves the tier at this size"""
    seen, meant, model = life12(vdb, "large-twelve")
    for kind in lc.NEWER_READS:                                      # four rounds of reads, each on the tier
        assert meant[(kind, "answered")] == 4 + (kind == "mmr") and seen["bf16_in_" + kind] == 4, (kind, seen, meant)
    # (the fifth MMR read is the one at m = 1024, B = 1: depth 1024 needs 240 (1024 + 192) = 291 840 rows for the tier -- an exact scan here)
    assert seen["mmr_pairs"] > 0 and seen["per_group_filled"] > 0 and seen["best_stage0"] > 0 and seen["best_list_searches"] > 0, seen
    assert seen["compactions"] >= 2 and seen["shrunk"] >= 1 and seen["grown_with_shadow"] >= 2, seen


@pytest.mark.parametrize("name", TWELVE_STORE_NAMES)
def test_store_lifecycle_twelve(vdb, name):
    """VectorStore.search_mmr, search_groups and recommend_best_batch beside the eight older store reads, with upserts, filters
    from the pool, the device filter from the start (early) or switched on mid-life (late: search_groups then sends the field's
    column up for the call alone, before), auto-compaction in the late one"""
    t = trace_of(name)
    ad = lc.GpuStoreAdapter(vdb, t["metric"], auto_compact=t["auto"])
    kinds = lc.Counter()
    try:
        lc.run(t, ad, expected=lc.slots(name, t), on_read=lambda step, op, model, args, got: kinds.update([(op[0], "error" in got)]))
    finally:
        ad.close()
    print(name, dict(ad.seen), dict(kinds))
    seen = ad.seen
    assert all(kinds[(k, False)] > 0 for k in lc.STORE_READS + lc.NEW_STORE_READS + lc.NEWER_STORE_READS), kinds
    assert any(e for (_, e) in kinds), kinds                                                   # a predicted error was met
    assert seen["mmr_pairs"] > 0 and seen["per_group_filled"] > 0 and seen["per_group_groups"] > 0 and seen["best_stage0"] > 0, seen
    assert seen["prefiltered_compiled"] > 0 and seen["compactions"] > 0, seen


@pytest.mark.parametrize("name", NEW_STORE_NAMES)
def test_store_lifecycle_with_numeric_fields(vdb, name):
    """VectorStore with the numeric fields ts and price: recommend_batch and search_batch_with_filters beside the six older
    reads, numeric filters compiled on the device table while the dictionary of ts grows on nearly every insert; in one schedule
    the device filter goes off and on again, and the new table must hold every number the old one had"""
    t = lc.store_pinned(name)
    ad = lc.GpuStoreAdapter(vdb, t["metric"], auto_compact=t["auto"])
    kinds = lc.Counter()
    try:
        lc.run(t, ad, expected=lc.slots(name, t), on_read=lambda step, op, model, args, got: kinds.update([(op[0], "error" in got)]))
    finally:
        ad.close()
    print(name, dict(ad.seen), dict(kinds))
    seen = ad.seen
    assert all(kinds[(k, False)] > 0 for k in lc.STORE_READS + lc.NEW_STORE_READS), kinds
    assert any(e for (_, e) in kinds), kinds                                                   # a predicted error was met
    assert seen["prefiltered_compiled"] > 0 and seen["grouped_scan"] > 0 and seen["grouped_unfiltered"] > 0 and seen["recommend_examples"] > 0, seen
    if name == "store-numeric-again":                                                          # compiled before AND after the table was rebuilt
        assert seen["table_switched_on"] == 2 and 0 < seen["prefiltered_compiled_on_a_second_table"] < seen["prefiltered_compiled"], seen


@pytest.mark.parametrize("name", STORE_NAMES)
def test_store_lifecycle(vdb, name):
    t = trace_of(name)
    ad = lc.GpuStoreAdapter(vdb, t["metric"], auto_compact=t["auto"])
    kinds = lc.Counter()
    lc.run(t, ad, expected=lc.slots(name, t), on_read=lambda step, op, model, args, got: kinds.update([(op[0], "error" in got)]))
    print(name, dict(ad.seen), dict(kinds))
    seen = ad.seen
    assert seen["prefiltered_compiled"] > 0 and seen["distinct"] > 0, seen
    assert (seen["prefiltered_host"] > 0) == (t["table_at"] == "mid"), seen
    assert seen["sparse_route"] > 0 and seen["by_id_struck"] + seen["by_id_cut"] > 0, seen
    assert seen["compactions"] > 0, seen
    assert all(kinds[(k, False)] > 0 for k in lc.STORE_READS), kinds
    assert any(e for (_, e) in kinds), kinds                                                   # a predicted error was met


# ------------------------------------------------------------------ the SPLIT row layout (lifecycle.SPLIT_PINNED)
SPLIT_NAMES = [p[0] for p in lc.SPLIT_PINNED]


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_split_lifecycle(vdb, name):
    """75 000 rows with the shadow off, all nine read kinds between add, upsert, remove, compact, a shrinking compaction refilled
    to the same row count, growth across re-allocations, a fall below 65 536 rows and back, a late non-finite row: every read
    against the model, and layout() = (layout, conversions) against the rule of DESIGN 4.3 after EVERY call
    (lifecycle.LayoutChecked; the only facts it takes from the engine are the read's own counters)."""
    t = lc.split_pinned(name)
    ad = lc.GpuIndexAdapter(vdb, t["metric"])
    checked = lc.LayoutChecked(ad)
    try:
        lc.run(t, checked, expected=lc.slots(name, t))
    finally:
        ad.close()
    rule, seen = checked.tracker.rule, ad.seen
    print(name, vars(rule), dict(seen))
    # conversions in both directions, a refusal, and a retry that holds: the schedule ends on SPLIT rows
    assert rule.forward >= 5 and rule.back >= 5 and rule.refusals == 1 and rule.expect()[0] == lc.LAYOUT_SPLIT, vars(rule)
    assert ad.ix.layout() == rule.expect()
    assert seen["route_bf16"] >= 20 and seen["bf16_large_k"] >= 2 and seen["bf16_shadow_rows"] == 0, seen
    assert seen["sparse_route"] >= 2 and seen["range_screened"] + seen["range_exact"] + seen["range_dense"] >= 12, seen
    assert seen["distinct_a"] > 0 and seen["grouped_scan"] > 0 and seen["grouped_unfiltered"] > 0 and seen["recommend_examples"] > 0, seen
    # (two re-allocations of a store that holds rows: 30 900 -> 75 000 and the refill after the shrinking compaction; the first
    # upload of 30 900 staged rows allocates, it does not grow)
    assert seen["numeric_compiles"] >= 3 and seen["grown"] >= 2 and seen["shrunk"] >= 1 and seen["compactions"] >= 4, seen

"""CPU proofs behind tests/test_gpu_discover.py (vdb_flat_discover_batch): the library exports the entry points;
the restatement of the list route -- one ranked list per request, the strike, the ranks, "k_b candidates of rank P or a complete
list", escalation -- gives the definition's answer on every family, metric and route (the proof that the answered rule is sound);
every family ends at the stage its name says, and each of the three stages is reached; and the argument checks refuse through the
library before anything touches a handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import discover_data as dd
from conftest import load_package

F32, U64, U32 = np.float32, np.uint64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vdb_flat_discover_batch", "vdb_flat_discover_batch_filtered", "vdb_flat_discover_stats", "vdb_flat_debug_set_discover_route")


def test_library_exports_and_ffi_declares_the_symbols():
    vdb = load_package()
    vdb.build()
    L = vdb._ffi.lib()
    header = open(os.path.join(ROOT, "include", "vdb_flat.h")).read()
    for name in NAMES:
        assert name in vdb._ffi.SYMBOLS
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "vdb_flat_discover_depth" in vdb._ffi.SYMBOLS and re.search(r"\bsize_t vdb_flat_discover_depth\(", header)
    assert len(L.vdb_flat_discover_batch.argtypes) == 14 and len(L.vdb_flat_discover_batch_filtered.argtypes) == 13
    assert re.search(r"#define VDB_DISCOVER_MAX_K %d\b" % dd.MAX_K, header)
    assert re.search(r"#define VDB_DISCOVER_MAX_PAIRS %d\b" % dd.MAX_PAIRS, header)
    # the contract names what is not built, the stage-0 formula and the row layout the scan reads
    for text in ("DISCOVERY SEARCH", "raw-vector target", "context-only", "sharded handles", "device-pointer", "HNSW", "SPLIT store converts back",
                 "max(2 k 2^P' + 2 P' + 1, 64)"):
        assert text in header, text
    assert L.vdb_abi_version() == 1
    for cls, names in ((vdb.GpuFlatIndex, ("discover_batch", "discover_stats", "debug_set_discover_route")),
                       (vdb.VectorStore, ("discover", "discover_batch"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_depth_values():
    L = load_package()._ffi.lib()
    d = L.vdb_flat_discover_depth
    for k, P, n in ((10, 0, 600), (10, 16, 600), (1, 0, 20), (1, 1, 100), (10, 3, 2000), (500, 16, 5000), (600, 16, 600), (10, 3, 66000),
                    (2 ** 64 - 1, 16, 3000), (10, 2, 0), (3, 2 ** 63, 5000)):
        for stage in (0, 1, 2, -1):
            assert d(k, P, n, stage) == dd.depth(k, P, n, stage), (k, P, n, stage)
    assert d(10, 0, 600, 0) == 64 and d(10, 16, 600, 0) == 600 and d(10, 3, 2000, 0) == 167 and d(500, 16, 5000, 0) == 1024
    assert d(10, 4, 1000000, 0) == 329 and d(1, 5, 1000000, 0) == 75 and d(1, 10, 5000, 0) == 1024
    assert d(1, 0, 20, 0) == 20 and d(10, 3, 66000, 1) == 1024 and d(10, 16, 600, 1) == 600 and d(10, 3, 66000, 2) == 0


@pytest.mark.parametrize("metric", dd.METRICS)
@pytest.mark.parametrize("name", sorted(dd.FAMILIES))
def test_lists_restatement_equals_the_definition(name, metric):
    rows, ids, reqs, k = dd.FAMILIES[name]()
    want = dd.definition("d-" + name, metric, rows, reqs, k, ids=ids)
    own = np.arange(len(rows), dtype=U64) if ids is None else ids
    for route in (dd.AUTO, dd.LISTS, dd.SCAN):
        got, stages, st = dd.lists_route("d-" + name, metric, rows, reqs, k, ids=ids, route=route)
        dd.same(got, want, (name, metric, route))
        assert st[2] + st[3] + st[4] == len(reqs) and st[0] == len(reqs) and st[1] == sum(2 * len(p) + 1 for _, p in reqs)
        if route == dd.SCAN:
            assert stages == [dd.STAGE_SCAN] * len(reqs) and st[6] == 0
    for (oi, dt, rank), req in zip(want, reqs):
        assert len(oi) == min(k, len(rows) - len(set(dd.examples(req))))
        assert not np.isin(oi, own[dd.examples(req)]).any()
        assert (rank <= len(req[1])).all() and (np.diff(rank.astype(np.int64)) <= 0).all()
        inside = np.diff(rank.astype(np.int64)) == 0                           # inside a rank level: ascending (ordered distance, id)
        od = dd.ordered(dt).astype(np.int64)
        assert ((np.diff(od) > 0) | ((np.diff(od) == 0) & (oi[1:] > oi[:-1])))[inside].all()


@pytest.mark.parametrize("metric", (dd.EUCLID, dd.COSINE))
def test_every_family_ends_at_the_stage_its_name_says_and_every_stage_is_reached(metric):
    reached = set()
    for name, by_request in sorted(dd.STAGES.items()):
        rows, ids, reqs, k = dd.FAMILIES[name]()
        want, stages, st = dd.expected("d-" + name, metric, rows, reqs, k, ids=ids)
        print(name, metric, "stages", stages, "stats", st)
        for b, stage in by_request.items():
            assert stages[b] == stage, (name, metric, b, stages)
            reached.add(stage)
    assert reached == {0, 1, dd.STAGE_SCAN}
    # half: about a hundred of the rows nearest the target fail the pair -- more than stage 0 looks at, fewer than stage 1 does
    rows, ids, reqs, k = dd.half()
    (oi, dt, rank), = dd.definition("d-half", metric, rows, reqs, k)
    full = dd.rb.ranking("d-half", metric, rows, 0, None, None)[0]
    at = int(np.nonzero(full == oi[0])[0][0])
    print("half", metric, "first rank-1 row at list position", at)
    assert dd.depth(k, 1, len(rows), 0) <= at < 1024 - k and (rank == 1).all()
    # deep: more than 1024 of them
    rows, ids, reqs, k = dd.deep()
    (oi, dt, rank), = dd.definition("d-deep", metric, rows, reqs, k)
    full = dd.rb.ranking("d-deep", metric, rows, 0, None, None)[0]
    assert int(np.nonzero(full == oi[0])[0][0]) > 1024 and (rank == 1).all()
    # contra: no row of rank P = 3, and the answer mixes levels
    rows, ids, reqs, k = dd.contra()
    want = dd.definition("d-contra", metric, rows, reqs, k)
    assert set(want[0][2].tolist()) == {2, 1} and len(want[0][0]) == k
    # loose: every row of the answer satisfies every pair; under Euclid the pairs change nothing among the rows near the target,
    # and the answer is the plain by-id answer
    rows, ids, reqs, k = dd.loose()
    want = dd.definition("d-loose", metric, rows, reqs, k)
    assert (want[0][2] == 3).all() and (want[1][2] == 1).all()
    if metric == dd.EUCLID:
        (pi, pd, _), = dd.definition("d-loose", metric, rows, [(reqs[0][0], ())], k + 2 * len(reqs[0][1]))
        assert np.array_equal(want[0][0], pi[~np.isin(pi, dd.examples(reqs[0]))][:k])


def test_restatement_under_a_mask_removed_rows_and_per_request_k():
    rows, ids, reqs, _ = dd.ragged()
    rng = np.random.default_rng(5)
    live = np.ones(len(rows), dtype=np.uint8)
    used = set(e for r in reqs for e in dd.examples(r))
    dead = [r for r in rng.choice(len(rows), 60, replace=False) if r not in used]
    live[dead] = 0
    mask = (rng.random(len(rows)) < 0.5).astype(np.uint8)
    flat = np.array(sorted(used))
    assert mask[flat].any() and not mask[flat].all()                           # some examples are masked out: still examples
    ks = [1 + (7 * b) % 23 for b in range(len(reqs))]
    ks[2] = 0
    for metric in dd.METRICS:
        want = dd.definition("d-ragged-lm", metric, rows, reqs, ks, live=live, mask=mask)
        for route in (dd.AUTO, dd.LISTS, dd.SCAN):
            got, _, _ = dd.lists_route("d-ragged-lm", metric, rows, reqs, ks, live=live, mask=mask, route=route)
            dd.same(got, want, (metric, route))
        for (oi, _, _), kb in zip(want, ks):
            assert len(oi) == kb and live[oi.astype(np.int64)].all() and mask[oi.astype(np.int64)].all()
    # k above the eligible rows: a short list that holds every one of them, and a complete list answers at stage 0
    tiny = rows[:40]
    reqs = ((3, ((4, 5), (6, 7))), (8, ()))
    want, stages, st = dd.expected("d-tiny", dd.EUCLID, tiny, reqs, 500, route=dd.LISTS)
    assert [len(w[0]) for w in want] == [35, 39] and list(stages) == [0, 0] and st[5] == 40


def test_an_equal_pair_is_never_satisfied_and_twins_tie_everywhere():
    rows, ids, reqs, k = dd.repeats()
    want = dd.definition("d-repeats", dd.EUCLID, rows, reqs, len(rows))
    assert (want[0][2] == 0).all() and (want[4][2] == 0).all()                 # (30, 30) and (t, t)
    assert set(want[1][2].tolist()) == {0, 2}                                  # the pair that stands twice counts twice or not at all
    assert want[0][0].size == len(rows) - 2 and want[4][0].size == len(rows) - 1   # the SET of examples is struck
    by_id = dd.definition("d-repeats", dd.EUCLID, rows, [(7, ())], len(rows))
    keep = by_id[0][0] != 30
    assert np.array_equal(want[0][0], by_id[0][0][keep]) and np.array_equal(want[0][1].view(U32), by_id[0][1][keep].view(U32))
    rows, ids, reqs, k = dd.tri()
    for metric in dd.METRICS:
        want = dd.definition("d-tri", metric, rows, reqs, len(rows), ids=ids)
        assert (want[0][2] == 0).all()                                         # d(p, x) == d(n, x) at every row: a tie is not satisfied
        oi, dt, rank = want[2]
        same_key = (rank[1:] == rank[:-1]) & (dt[1:].view(U32) == dt[:-1].view(U32))
        assert same_key.sum() > len(oi) // 2 and (oi[1:][same_key] > oi[:-1][same_key]).all()   # equal (rank, distance): the id decides
    D0 = dd.depth(dd.K, 2, len(rows), 0)
    od = dd.rb.ranking("d-tri", dd.EUCLID, rows, reqs[1][0], ids, None)[1]
    assert od[D0 - 1] == od[D0] or od[D0 - 1] == od[D0 - 2]                    # the list ends inside a run of equal distances


def test_inf_family():
    rows, ids, reqs, k = dd.inf_family()
    want = dd.definition("d-inf", dd.EUCLID, rows, reqs, k)
    for route in (dd.LISTS, dd.SCAN):
        got, stages, _ = dd.lists_route("d-inf", dd.EUCLID, rows, reqs, k, route=route)
        dd.same(got, want, route)
    oi, dt, rank = want[0]
    assert len(oi) == dd.INF_N - 3 and np.isinf(dt).sum() == len(dd.INF_ROWS)  # +inf target distances are distances, not errors
    oi, dt, rank = want[1]
    at = {int(x): int(r) for x, r in zip(oi, rank)}
    # pair (inf row, 9): inf < finite never; pair (9, inf row): finite < inf at finite rows, NaN at the other +inf rows
    assert at[dd.INF_ROWS[2]] == 0 and at[20] >= 1 and len(oi) == dd.INF_N - 5
    with pytest.raises(dd.NanDistance):
        dd.definition("d-inf", dd.EUCLID, rows, dd.inf_nan_request(), dd.K)


def test_argument_checks_refuse_before_any_handle_is_touched():
    vdb = load_package()
    L = vdb._ffi.lib()
    bad = vdb._ffi.ERR_INVALID_ARGUMENT
    szp, u64p = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint64)

    def call(targets, pair_ids, offsets, nq, filtered=False, no_pairs=False, no_targets=False):
        tg = np.asarray(targets, dtype=U64)
        pr = np.asarray(pair_ids, dtype=U64)
        off = np.asarray(offsets, dtype=np.uintp)
        oi, od, orank, oc = np.zeros(4, dtype=U64), np.zeros(4, dtype=F32), np.zeros(4, dtype=U32), np.zeros(4, dtype=np.uintp)
        head = (None, None if no_targets else tg.ctypes.data_as(u64p), None if no_pairs else pr.ctypes.data_as(u64p), off.ctypes.data_as(szp),
                nq, None, 1)
        tail = (1, oi.ctypes.data_as(u64p), od.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                orank.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), oc.ctypes.data_as(szp))
        if filtered:
            rc = L.vdb_flat_discover_batch_filtered(*head, ctypes.c_void_p(16), *tail)   # (never dereferenced: the checks come first)
        else:
            rc = L.vdb_flat_discover_batch(*head, None, 0, *tail)
        return rc, vdb._ffi.last_error()[0]

    # the handle is NULL throughout: every refusal below names the ARGUMENT, so it came before the handle was looked at
    for filtered in (False, True):
        rc, msg = call([1], [2, 3], [1, 2], 1, filtered)
        assert rc == bad and "offsets[0]" in msg, msg
        rc, msg = call([1, 2], [2, 3, 4, 5], [0, 2, 1], 2, filtered)
        assert rc == bad and "decrease" in msg, msg
        rc, msg = call([1], list(range(34)), [0, 17], 1, filtered)
        assert rc == bad and "more than 16" in msg, msg
        rc, msg = call([1, 2], list(range(40)), [0, 3, 20], 2, filtered)
        assert rc == bad and "request 1 has 17 pairs" in msg, msg
        rc, msg = call([1], [2, 3], [0, 1], 1, filtered, no_pairs=True)
        assert rc == bad and "null argument" in msg, msg
        rc, msg = call([1], [2, 3], [0, 1], 1, filtered, no_targets=True)
        assert rc == bad and "null argument" in msg, msg
        rc, msg = call([1], list(range(32)), [0, 16], 1, filtered)
        assert rc == bad and "null argument" in msg, msg                       # 16 pairs are fine: now the handle
    out = (ctypes.c_uint64 * 8)()
    assert L.vdb_flat_discover_stats(None, out) == bad
    assert L.vdb_flat_debug_set_discover_route(None, 0) == bad
    oc = np.zeros(1, dtype=np.uintp)
    assert L.vdb_flat_discover_batch_filtered(None, None, None, None, 0, None, 1, None, 1, None, None, None, oc.ctypes.data_as(szp)) == bad

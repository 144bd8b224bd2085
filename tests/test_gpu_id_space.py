"""Everything a result owes to its ids, on every search path, over the whole uint64 id range (tests/id_families.py).

The sharpest statement: for the same rows and queries, relabelling the rows by an increasing map f must give ids equal to
f(control ids), the same distance bits, the same counts and the same tier counters.  The control run and every family are also
compared with the oracle directly (it orders ties by unsigned id: tests/test_id_space_cpu.py).  Tolerance 0 everywhere.

The tie data repeats a base block R > k times and asks for base rows, so that every row such a query returns is chosen by
its id alone; the copies of one row lie nb rows apart, so one tie group spans every tile, every workgroup's sub-pool and every
shard.  The gaussian data keeps the certified fast path busy; its first queries sit next to the rows that carry the largest
label (2^64 - 1 in `top`) and the labels around the middle (where across32 / across63 wrap), in both row orders."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from conftest import ROOT, load_package
from id_families import FAMILIES, ORDERS, RELABELLED, build_cpp_id_space_test, family_ids, lexsort_u64, permutation

pytestmark = pytest.mark.gpu

COUNTERS = ("bf16_screen", "uncertified", "f32_tier_queries", "rethreshold_queries", "exact_queries", "pool_overflows", "mfma_queries")
METRICS = [0, 1, 2]


def _const(name):
    """A constexpr of csrc/vdb_index.h that no accessor exports (the numbers are not copied into this file)."""
    with open(os.path.join(ROOT, "vectordb-from-scratch_amd", "csrc", "vdb_index.h")) as f:
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, f.read())
    return int(m.group(1))


SMALL_N, DIRECT_MAX_Q, MAX_SELECT, SUPER = _const("SMALL_N"), _const("DIRECT_MAX_Q"), _const("MAX_SELECT"), _const("SUPER")
BF16_MIN_ROWS, BF16_MAX_K = _const("BF16_MIN_ROWS"), _const("BF16_MAX_K")

_INDEXES = {}
_ORACLE = {}


@pytest.fixture(scope="module")
def vdb():
    v = load_package()
    v.build()
    yield v
    _INDEXES.clear()
    _ORACLE.clear()


# ------------------------------------------------------------------ data
class Data:
    def __init__(self, name, rows, q, tie_queries):
        self.name, self.rows, self.q, self.tie_queries = name, np.ascontiguousarray(rows), np.ascontiguousarray(q), tie_queries
        self.n = rows.shape[0]

    def labels(self, order):
        return None if order == "row" else permutation(self.n)


def tie_data(name, nb, R, d, nq, seed, n=None):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((nb, d)).astype(np.float32)
    rows = np.concatenate([base] * R, 0)[:n]
    return Data(name, rows, base[np.arange(nq) % nb] + 0.0, True)


def gauss_data(name, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    inv = np.argsort(permutation(n))                                    # inv[label] = the row that carries it in the perm order
    targets = [n - 1, inv[n - 1], n // 2, inv[n // 2], n // 2 - 1, inv[n // 2 - 1], 0, inv[0]][:nq]
    for i, r in enumerate(targets):
        q[i] = rows[r] + 0.01 * q[i]
    return Data(name, rows, q, False)


def oracle_search(data, metric, family, order, k, b, ids, live=None, tag=""):
    key = (data.name, metric, family, order, k, b, tag)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.flat_search(metric, data.rows, data.q[b], k, ids=ids, live=live)
    return _ORACLE[key]


def assert_ids_decide(data, metric, k, nq):
    """From the oracle's output alone, before any GPU call: at least k + 1 rows share the k-th distance of every tie query."""
    assert data.tie_queries
    ids = FAMILIES["control"](data.n)
    for b in sorted({0, nq // 2, nq - 1}):
        oi, od = oracle_search(data, metric, "control", "row", k + 1, b, ids)
        assert len(od) == k + 1 and od[k - 1].view(np.uint32) == od[k].view(np.uint32), (data.name, metric, k, b)


def index_for(vdb, data, metric, family, order, devices=None, shadow=False, cache=True):
    key = (data.name, metric, family, order, tuple(devices) if devices else None, shadow)
    if key in _INDEXES:
        return _INDEXES[key]
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, devices=devices)
    if shadow:
        ix.set_shadow(True)
    ids = family_ids(family, data.n, data.labels(order))
    ix.add_bulk(data.rows, ids=ids)
    if cache:
        _INDEXES[key] = (ix, ids)
    return ix, ids


def counters(st):
    return {c: st[c] for c in COUNTERS}


def check_rows(got, b, oi, od, what):
    gi, gd, gc = got
    assert gc[b] == len(oi), (what, b, int(gc[b]), len(oi))
    assert np.array_equal(gi[b, :len(oi)], oi), (what, b, gi[b, :len(oi)], oi)
    assert np.array_equal(gd[b, :len(oi)].view(np.uint32), od.view(np.uint32)), (what, b)


def sweep(vdb, data, metric, k, nq=None, configure=None, expect=None, families=RELABELLED, orders=ORDERS, devices=None,
          shadow=False, cache=True, labels_of=None):
    """The relabelling claim for one path: `configure(ix)` puts the index on the path (and returns an undo), `expect(st, nq)`
    asserts from last_stats() that the path really answered."""
    nq = data.q.shape[0] if nq is None else nq
    q = data.q[:nq]
    qsel = sorted({0, 1, nq // 2, nq - 1} & set(range(nq)))
    for order in orders:
        runs = {}
        for family in ["control"] + list(families):
            ix, ids = index_for(vdb, data, metric, family, order, devices, shadow, cache)
            undo = configure(ix) if configure else None
            try:
                res = ix.search_batch_arrays(q, k)
                st = ix.last_stats()
            finally:
                if undo:
                    undo()
            if expect:
                expect(st, nq)
            what = (data.name, metric, family, order, k, nq)
            for b in qsel:
                oi, od = oracle_search(data, metric, family, order, k, b, ids)
                check_rows(res, b, oi, od, what)
            runs[family] = (res, counters(st))
            if family != "control":
                (ci, cd, cc), cst = runs["control"]
                gi, gd, gc = res
                f = FAMILIES[family](data.n)
                assert np.array_equal(gc, cc), what
                assert counters(st) == cst, (what, counters(st), cst)
                for b in range(nq):
                    c = int(cc[b])
                    assert np.array_equal(gi[b, :c], f[ci[b, :c].astype(np.int64)]), (what, b)
                    assert np.array_equal(gd[b, :c].view(np.uint32), cd[b, :c].view(np.uint32)), (what, b)
            if not cache:
                del ix


def tiers(flags):
    def configure(ix):
        ix.set_tiers(flags)
        return lambda: ix.set_tiers(0)
    return configure


def screen_off(ix):
    ix.set_screen(0)
    return lambda: ix.set_screen(1)


# ------------------------------------------------------------------ the direct path of small indexes
def small_sets():
    n = SMALL_N // 2
    return [tie_data("small_ties", n // 512, 512, 24, DIRECT_MAX_Q, 101), gauss_data("small_gauss", n, 24, DIRECT_MAX_Q, 102)]


@pytest.mark.parametrize("metric", METRICS)
def test_direct_path_of_small_indexes(vdb, metric):
    for data in small_sets():
        for k in (10, 300):                                             # the two `keep` modes of the select: k < 256, k >= 256
            if data.tie_queries:
                assert_ids_decide(data, metric, k, DIRECT_MAX_Q)

            def direct(st, nq):
                assert st["exact_queries"] == nq and st["bf16_screen"] == 0, st
            sweep(vdb, data, metric, k, expect=direct)
            sweep(vdb, data, metric, k, configure=tiers(vdb.GpuFlatIndex.TIERS_NO_DIRECT))


# ------------------------------------------------------------------ the f32 tier alone
@pytest.mark.parametrize("metric", METRICS)
def test_f32_tier_small_and_fused(vdb, metric):
    def f32_only(st, nq):
        assert st["bf16_screen"] == 0, st
    n = SMALL_N // 2
    for data in (tie_data("small_ties_b", n // 512, 512, 24, 40, 103), gauss_data("small_gauss_b", n, 24, 40, 104)):
        if data.tie_queries:
            assert_ids_decide(data, metric, 10, 40)
        sweep(vdb, data, metric, 10, configure=screen_off, expect=f32_only)          # n <= SMALL_N, more than DIRECT_MAX_Q queries
    n = SMALL_N + 4096
    for data in (tie_data("fused_ties", n // 512, 512, 16, SUPER, 105), gauss_data("fused_gauss", n, 16, SUPER, 106)):
        if data.tie_queries:
            assert_ids_decide(data, metric, 10, SUPER)

        def fused(st, nq):
            assert st["bf16_screen"] == 0 and st["rows_scanned"] >= data.n, st
        for nq in (20, 40, 100, SUPER):                                  # the 32-, 64-, 128- and 256-query kernel shapes
            sweep(vdb, data, metric, 10, nq=nq, configure=screen_off, expect=fused)


# ------------------------------------------------------------------ the screening tier and the forced hand-overs
def screen_sets():
    n = BF16_MIN_ROWS
    return [tie_data("screen_ties", n // 512, 512, 64, 2 * SUPER + 88, 107), gauss_data("screen_gauss", n, 64, 2 * SUPER + 88, 108)]


@pytest.mark.parametrize("shadow", [False, True], ids=["f32_rows", "bf16_shadow"])
@pytest.mark.parametrize("metric", METRICS)
def test_screening_tier(vdb, metric, shadow):
    for data in screen_sets():
        if data.tie_queries:
            assert_ids_decide(data, metric, 10, data.q.shape[0])

        def screened(st, nq):
            assert st["bf16_screen"] == 1 and st["shadow_rows"] == (1 if shadow else 0), st
            if not data.tie_queries:
                assert st["exact_queries"] == 0 and st["pool_overflows"] == 0, st    # gaussian rows: the certified fast path answers
        for nq in (40, SUPER + 44, 2 * SUPER + 88):                      # one pass; the wide kernel; two streams
            sweep(vdb, data, metric, 10, nq=nq, expect=screened, shadow=shadow)


@pytest.mark.parametrize("metric", METRICS)
def test_forced_f32_and_forced_exact(vdb, metric):
    for data in screen_sets():
        def forced_f32(st, nq):
            assert st["bf16_screen"] == 1 and st["f32_tier_queries"] == nq, st

        def forced_exact(st, nq):
            assert st["exact_queries"] == nq, st
        sweep(vdb, data, metric, 10, nq=40, configure=tiers(vdb.GpuFlatIndex.TIERS_FORCE_F32), expect=forced_f32)
        sweep(vdb, data, metric, 10, nq=40, configure=tiers(vdb.GpuFlatIndex.TIERS_FORCE_EXACT), expect=forced_exact)


# ------------------------------------------------------------------ the re-threshold pass
@pytest.mark.parametrize("metric", METRICS)
def test_rethreshold_pass(vdb, metric):
    """The data and the assertion of test_rethreshold_pass_answers_what_the_depth_limit_could_not (tests/test_gpu_screen.py),
    so that rerank_all_kernel is the kernel that answered.  In the perm order the largest label (2^64 - 1 in `top`) is put on
    the row the oracle names as query 0's nearest, the middle label (where across32 / across63 wrap) on its second nearest:
    the ids the kernels could mistake sit inside the first k."""
    rng = np.random.default_rng(28)
    n, d = 120000, 96
    rows = rng.standard_normal((n, d)).astype(np.float32)
    centre = rng.standard_normal(d).astype(np.float32) * 2.0
    rows[40000:40600] = centre + 1e-3 * rng.standard_normal((600, d)).astype(np.float32)
    q = (centre + 1e-4 * rng.standard_normal((5, d))).astype(np.float32)
    data = Data("rethreshold_%d" % metric, rows, q, False)
    near = oracle.flat_search(metric, rows, q[0], 2)[0].astype(np.int64)     # ids = row numbers here
    lab = permutation(n)
    for row, label in ((near[0], n - 1), (near[1], n // 2)):
        other = int(np.nonzero(lab == label)[0][0])
        lab[other], lab[row] = lab[row], label
    data.labels = lambda order: None if order == "row" else lab

    def rethresholded(st, nq):
        assert st["bf16_screen"] == 1 and st["rethreshold_queries"] == 5 and st["f32_tier_queries"] == 0 and st["exact_queries"] == 0, st
    sweep(vdb, data, metric, 10, expect=rethresholded, cache=False)


# ------------------------------------------------------------------ large k and its exact-scan fallback
@pytest.mark.parametrize("metric", METRICS)
def test_large_k_and_its_exact_fallback(vdb, metric):
    k = 300
    assert BF16_MAX_K < k
    n = int(vdb._ffi.lib().vdb_flat_large_k_min_rows(k))
    nb = (n + 511) // 512
    for data in (tie_data("large_k_ties", nb, 512, 16, 12, 109), gauss_data("large_k_gauss", nb * 512, 16, 12, 110)):
        if data.tie_queries:
            assert_ids_decide(data, metric, k, 12)

        def screened(st, nq):
            assert st["bf16_screen"] == 1, st

        def fallback(st, nq):
            assert st["bf16_screen"] == 0, st

        def large_k_off(ix):
            ix.set_large_k(False)
            return lambda: ix.set_large_k(True)
        sweep(vdb, data, metric, k, expect=screened)
        sweep(vdb, data, metric, k, configure=large_k_off, expect=fallback)


# ------------------------------------------------------------------ the chunked exact emit (k > MAX_SELECT)
@pytest.mark.parametrize("metric", METRICS)
def test_chunked_exact_emit_across_tie_groups(vdb, metric):
    """Three rows, each MAX_SELECT * 3 / 4 times: the groups of equal distances straddle positions MAX_SELECT and 2 * MAX_SELECT
    of the result, so "strictly above the previous chunk's last key" is decided by the id rank."""
    R = MAX_SELECT * 3 // 4
    data = tie_data("chunked_ties", 3, R, 8, 3, 111)
    k = 2 * MAX_SELECT + R // 4
    assert R < MAX_SELECT < 2 * R < 2 * MAX_SELECT < k < 3 * R
    assert_ids_decide(data, metric, k, 3)
    assert_ids_decide(data, metric, MAX_SELECT, 3)
    for b in range(3):                                                    # the three groups really are three distances
        od = oracle_search(data, metric, "control", "row", k + 1, b, FAMILIES["control"](data.n))[1]
        assert len(set(od.view(np.uint32).tolist())) == 3

    def not_screened(st, nq):
        assert st["bf16_screen"] == 0, st
    sweep(vdb, data, metric, k, expect=not_screened)
    sweep(vdb, data, metric, MAX_SELECT + 1, expect=not_screened)


# ------------------------------------------------------------------ the id mask
def _mask(bits, seed):
    rng = np.random.default_rng(seed)
    on = rng.random(bits) < 0.5
    on[:4096] = True                  # an id that wrapped at 2^32 or 2^64 into the low bits would read a SET bit
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    return on, np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64)


@pytest.mark.parametrize("metric", METRICS)
def test_id_mask_high_ids_are_ineligible_and_do_not_wrap(vdb, metric):
    n = SMALL_N + 4096
    for data in (tie_data("fused_ties", n // 512, 512, 16, SUPER, 105), gauss_data("fused_gauss", n, 16, SUPER, 106)):
        nq, k = 12, 10
        q = data.q[:nq]
        mask_bits = 3 * data.n
        on, mask = _mask(mask_bits, 5)
        for order in ORDERS:
            lab = data.labels(order)
            for family in FAMILIES:
                ix, ids = index_for(vdb, data, metric, family, order)
                res = ix.search_batch_arrays(q, k, id_mask=mask, mask_bits=mask_bits)
                if family == "control":
                    live = on[ids.astype(np.int64)].astype(np.uint8)
                    for b in (0, 1, nq - 1):
                        oi, od = oracle_search(data, metric, family, order, k, b, ids, live=live, tag="mask")
                        check_rows(res, b, oi, od, (data.name, family, order))
                else:
                    assert int(ids.min()) >= mask_bits
                    assert np.all(res[2] == 0), (data.name, metric, family, order, res[2])
            # half control ids, half high ids: the high half is ineligible, the low half is selected as before
            for family in ("across32", "top"):
                mixed = np.where(np.arange(data.n) < data.n // 2, FAMILIES["control"](data.n), FAMILIES[family](data.n))
                ids = mixed if lab is None else np.ascontiguousarray(mixed[lab])
                ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
                ix.add_bulk(data.rows, ids=ids)
                low = ids < np.uint64(mask_bits)
                live = np.zeros(data.n, dtype=np.uint8)
                live[low] = on[ids[low].astype(np.int64)]
                assert 0 < int(live.sum()) < int(low.sum()) == data.n // 2
                for kw in ({}, {"tiers": ix.TIERS_FORCE_EXACT}):
                    ix.set_tiers(kw.get("tiers", 0))
                    res = ix.search_batch_arrays(q, k, id_mask=mask, mask_bits=mask_bits)
                    ix.set_tiers(0)
                    for b in range(nq):
                        oi, od = oracle.flat_search(metric, data.rows, q[b], k, ids=ids, live=live)
                        check_rows(res, b, oi, od, (data.name, "mixed " + family, order))
                unm = ix.search_batch_arrays(q, k)                       # and unmasked the high half is found as usual
                for b in (0, nq - 1):
                    oi, od = oracle.flat_search(metric, data.rows, q[b], k, ids=ids)
                    check_rows(unm, b, oi, od, (data.name, "mixed unmasked " + family, order))


# ------------------------------------------------------------------ mutation by id, then compact()
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("layout", ["row", "perm", "monotone_after_compact"])
def test_mutation_by_id_and_compaction(vdb, family, layout):
    """remove / overwrite / get_vector / len by id, searches before and after compact() -- which recomputes ids_monotone: the
    `monotone_after_compact` layout is out of order in exactly two rows, both removed; the `perm` layout stays out of order."""
    metric, n, d, k = 0, 600, 8, 40
    rng = np.random.default_rng(17)
    base = rng.standard_normal((20, d)).astype(np.float32)
    rows = np.concatenate([base] * 30, 0)                                # tie groups of 30 < k: the cut falls inside the second group
    q = base[:4] + 0.0
    lab = np.arange(n)
    if layout == "perm":
        lab = permutation(n)
    elif layout == "monotone_after_compact":
        lab[10], lab[500] = lab[500], lab[10]
    ids = family_ids(family, n, lab)
    ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False)
    ix.add_bulk(rows, ids=ids)
    live = np.ones(n, dtype=np.uint8)
    dead = sorted({10, 500, 0, n - 1, int(np.nonzero(lab == n - 1)[0][0]), int(np.nonzero(lab == n // 2)[0][0]),
                   int(np.nonzero(lab == n // 2 - 1)[0][0])} | set(range(3, n, 7)))
    for r in dead:
        ix.remove(int(ids[r]))
        live[r] = 0
    ix.remove(int(ids[dead[0]]))                                          # a second remove and an absent id are Ok
    assert ix.len() == int(live.sum())
    for r in (1, 2, n - 2, dead[0], dead[-1]):
        v = ix.get_vector(int(ids[r]))
        assert (v is None) if not live[r] else np.array_equal(v.data, rows[r]), r
    all_rows, all_ids = rows, ids
    if layout != "monotone_after_compact":                               # overwrite by id: the old row dies, the new one is appended
        over = [1, 2, n - 2]
        new = rng.standard_normal((len(over), d)).astype(np.float32)
        new[0] = base[0]                                                 # joins query 0's tie group under its old id
        for r, v in zip(over, new):
            ix.add(int(ids[r]), vdb.Vector(v))
            live[r] = 0
        all_rows = np.concatenate([rows, new], 0)
        all_ids = np.concatenate([ids, ids[over]])
        live = np.concatenate([live, np.ones(len(over), dtype=np.uint8)])
        assert np.array_equal(ix.get_vector(int(ids[1])).data, new[0])
    assert ix.len() == int(live.sum())

    def searches():
        out = []
        for flags in (0, ix.TIERS_NO_DIRECT, ix.TIERS_FORCE_EXACT):
            ix.set_tiers(flags)
            res = ix.search_batch_arrays(q, k)
            ix.set_tiers(0)
            for b in range(4):
                oi, od = oracle.flat_search(metric, all_rows, q[b], k, ids=all_ids, live=live)
                check_rows(res, b, oi, od, (family, layout, flags))
            out.append(res)
        return out
    before = searches()
    assert ix.compact() == int((live == 0).sum())
    assert ix.len() == int(live.sum())
    after = searches()
    for x, y in zip(before, after):
        assert all(np.array_equal(a.view(np.uint8), c.view(np.uint8)) for a, c in zip(x, y))
    alive = int(np.nonzero(live[:n])[0][3])
    assert ix.get_vector(int(ids[dead[0]])) is None and np.array_equal(ix.get_vector(int(ids[alive])).data, rows[alive])


# ------------------------------------------------------------------ two searches in flight
def test_submit_wait_carries_the_top_ids(vdb):
    import torch
    data = screen_sets()[1]
    ix, ids = index_for(vdb, data, 1, "top", "perm")
    dev = torch.device("cuda", 0)
    k, B = 10, 64
    qs = [torch.from_numpy(data.q[i * B:(i + 1) * B]).to(dev) for i in range(2)]
    outs = [(torch.empty((B, k), dtype=torch.int64, device=dev), torch.empty((B, k), dtype=torch.float32, device=dev),
             torch.empty((B,), dtype=torch.int32, device=dev)) for _ in range(2)]
    t = [ix.search_batch_device_submit(qs[i].data_ptr(), B, data.q.shape[1], k, outs[i][0].data_ptr(), outs[i][1].data_ptr(), outs[i][2].data_ptr())
         for i in range(2)]
    for x in t:
        ix.search_batch_device_wait(x)
    torch.cuda.synchronize()
    for i in range(2):
        gi, gd, gc = ix.search_batch_arrays(data.q[i * B:(i + 1) * B], k)
        assert np.array_equal(outs[i][0].cpu().numpy().view(np.uint64), gi)
        assert np.array_equal(outs[i][1].cpu().numpy().view(np.uint32), gd.view(np.uint32))
        assert np.array_equal(outs[i][2].cpu().numpy(), gc.astype(np.int32))
    for b in (0, 1):                                                      # the queries next to the row whose id is 2^64 - 1
        oi, od = oracle_search(data, 1, "top", "perm", k, b, ids)
        assert np.array_equal(outs[0][0].cpu().numpy().view(np.uint64)[b], oi)
    assert int(ids.max()) == 2 ** 64 - 1 and int(ids.max()) in {int(x) for x in outs[0][0].cpu().numpy().view(np.uint64)[:2].ravel()}


# ------------------------------------------------------------------ the sharded handle
def _device_lists():
    import torch
    lists = [[0], [0, 0, 0]]                                             # one GPU listed for several shards: the peer exchange
    if torch.cuda.device_count() > 1:
        lists.append(list(range(torch.cuda.device_count())))
    return lists


@pytest.mark.parametrize("metric", METRICS)
def test_sharded_handle_tie_groups_span_the_shards(vdb, metric):
    n = SMALL_N + 4096
    for data in (tie_data("fused_ties", n // 512, 512, 16, SUPER, 105), gauss_data("fused_gauss", n, 16, SUPER, 106)):
        if data.tie_queries:
            assert_ids_decide(data, metric, 10, 24)
        for devices in _device_lists():
            sweep(vdb, data, metric, 10, nq=24, families=("across63", "top"), devices=devices, cache=False)
            ix, ids = index_for(vdb, data, metric, "top", "perm", devices, cache=False)
            plain, _ = index_for(vdb, data, metric, "top", "perm")
            a, b = ix.search_batch_arrays(data.q[:24], 10), plain.search_batch_arrays(data.q[:24], 10)
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
            assert ix.shards() == len(devices)


def test_one_rank_shard_group_exchange_carries_the_top_ids(vdb):
    """The packed layout end to end (launch_merge_packed through the shard group's one-rank exchange)."""
    import torch
    from vectordb_from_scratch_amd.sharded import ShardGroup, group_search
    data = screen_sets()[0]
    grp = ShardGroup(ShardGroup.unique_id(), 0, 1, device=0)
    for family in ("across63", "top"):
        ix, ids = index_for(vdb, data, 0, family, "perm")
        q = data.q[:6]
        gi, gd, gc = (t.cpu().numpy() for t in group_search(grp, ix)(torch.from_numpy(q).to(torch.device("cuda", 0)), 10))
        pi, pd, pc = ix.search_batch_arrays(q, 10)
        assert np.array_equal(gi.view(np.uint64), pi) and np.array_equal(gd.view(np.uint32), pd.view(np.uint32)) and np.all(gc == 10)
        for b in (0, 5):
            oi, od = oracle_search(data, 0, family, "perm", 10, b, ids)
            assert np.array_equal(gi.view(np.uint64)[b], oi)


# ------------------------------------------------------------------ the merge kernels alone
def _merge_parts(family, W, B, k, seed):
    rng = np.random.default_rng(seed)
    N = W * B * k
    ids = family_ids(family, N, rng.permutation(N)).reshape(W, B, k)
    d = (rng.integers(0, 5, (W, B, k)) * 0.5).astype(np.float32)          # equal distances within and across the parts
    counts = rng.integers(k // 2, k + 1, (W, B)).astype(np.int32)
    counts[1, 0], counts[2, 0], counts[0, 1] = 1, 0, k                    # short parts
    p, b, j = (int(x[0]) for x in np.nonzero(ids == ids.max()))
    d[p, b, j] = -1.0                                                     # the largest id (2^64 - 1 in `top`) is a real, first entry
    counts[p, b] = max(counts[p, b], 1)
    for pp in range(W):
        for bb in range(B):
            o = lexsort_u64(ids[pp, bb], d[pp, bb])
            ids[pp, bb], d[pp, bb] = ids[pp, bb][o], d[pp, bb][o]
    return ids, d, counts


@pytest.mark.parametrize("family", ["across63", "top", "high_word_only", "low_word_only"])
@pytest.mark.parametrize("W,k", [(4, 64), (8, 300)])
def test_merge_kernels_order_by_unsigned_id(vdb, family, W, k):
    import torch
    from vectordb_from_scratch_amd.sharded import merge_topk_hip
    assert (W * k <= MAX_SELECT) == (k == 64)                             # the LDS sort and the rank merge
    B = 5
    ids, d, counts = _merge_parts(family, W, B, k, W * k)
    dev = torch.device("cuda", 0)
    gi, gd, gc = merge_topk_hip(torch.from_numpy(ids.view(np.int64)).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(counts).to(dev), k)
    torch.cuda.synchronize()
    gi, gd, gc = gi.cpu().numpy().view(np.uint64), gd.cpu().numpy(), gc.cpu().numpy()
    # the packed all-gather layout: ids int64[B*k] | dists f32[B*k] | counts i32[B] | status i32 | pad
    nk = B * k
    words = B * (3 * k + 1) + 1
    words += words & 1
    packed = np.zeros((W, words), dtype=np.int32)
    for p in range(W):
        packed[p, :2 * nk] = ids[p].reshape(-1).view(np.int32)
        packed[p, 2 * nk:3 * nk] = d[p].reshape(-1).view(np.int32)
        packed[p, 3 * nk:3 * nk + B] = counts[p]
    pk = torch.from_numpy(packed).to(dev)
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oc = torch.empty((B,), dtype=torch.int32, device=dev)
    os_ = torch.zeros((1,), dtype=torch.int32, device=dev)
    rc = vdb._ffi.lib().vdb_merge_topk_packed_device(0, ctypes.c_void_p(pk.data_ptr()), W, words, B, k, ctypes.c_void_p(oi.data_ptr()),
                                                     ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(oc.data_ptr()),
                                                     ctypes.c_void_p(os_.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0
    pi, pd, pc = oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy()
    import sharded_mirror                                                # the corrected torch mirror agrees with the device merge
    ti, td, tc = sharded_mirror.merge_topk_torch(torch.from_numpy(ids.view(np.int64)), torch.from_numpy(d), torch.from_numpy(counts), k)
    assert np.array_equal(tc.numpy(), gc)
    for b in range(B):
        assert np.array_equal(ti[b, :gc[b]].numpy().view(np.uint64), gi[b, :gc[b]]) and np.array_equal(td[b, :gc[b]].numpy().view(np.uint32), gd[b, :gc[b]].view(np.uint32))
    saw_max = False
    for b in range(B):
        ii = np.concatenate([ids[p, b, :counts[p, b]] for p in range(W)])
        dd = np.concatenate([d[p, b, :counts[p, b]] for p in range(W)])
        o = lexsort_u64(ii, dd)[:k]
        for got_i, got_d, got_c in ((gi, gd, gc), (pi, pd, pc)):
            assert got_c[b] == len(o), (b, got_c[b], len(o))
            assert np.array_equal(got_i[b, :len(o)], ii[o]), b
            assert np.array_equal(got_d[b, :len(o)].view(np.uint32), dd[o].view(np.uint32)), b
        saw_max = saw_max or int(ids.max()) in {int(x) for x in ii[o]}
    assert saw_max


# ------------------------------------------------------------------ the store and the server
def test_store_and_server_round_trip_external_ids_above_53_bits(vdb):
    """External ids are strings end to end (storage.rs:83-96, routes.rs:330-385), so an id whose value needs more than 53 bits
    is never a JSON number and cannot be rounded: it comes back character for character."""
    import json
    from starlette.testclient import TestClient
    from vectordb_from_scratch_amd.server import AppState, create_app
    ext = [str(int(x)) for x in FAMILIES["top"](64)]
    st = vdb.VectorStore(vdb.DistanceMetric.Euclidean)
    client = TestClient(create_app(AppState(st)))
    r = client.post("/vectors/batch", json={"vectors": [{"id": e, "vector": [float(i // 8), 1.0]} for i, e in enumerate(ext)]})
    assert r.status_code == 201 and r.json() == {"inserted": 64}
    r = client.post("/search/batch", json={"queries": [{"vector": [0.0, 1.0], "k": 12}, {"vector": [7.0, 1.0], "k": 8}]})
    assert r.status_code == 200
    body = json.loads(r.text)
    assert [x["id"] for x in body[0]] == ext[:12] and [x["id"] for x in body[1]] == ext[56:64]
    assert body[1][-1]["id"] == str(2 ** 64 - 1)


# ------------------------------------------------------------------ HNSW
def test_hnsw_refuses_ids_it_cannot_hold(vdb):
    """include/vdb_hnsw.h: node ids at or above 2^32 - 16 are refused with VDB_ERR_INVALID_ARGUMENT at add time -- by add and by
    build_batch, before anything of the batch is inserted -- and never truncated; the graph of the ids it holds stays equal to
    the CPU restatement's, and the calls that only look an id up treat such an id as absent."""
    rng = np.random.default_rng(41)
    n, d = 400, 16
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((8, d)).astype(np.float32)
    small = np.arange(n, dtype=np.uint64) * 3 + 1
    h = vdb.GpuHnswIndex(vdb.DistanceMetric.Euclidean, vdb.HnswParams.new(8, 60, 40), seed=9)
    o = oracle.HnswOracle(0, m=8, ef_construction=60, ef_search=40, seed=9)
    h.build_batch((small[:300], rows[:300]))
    for i in range(300):
        o.insert(int(small[i]), rows[i])
    limit = 2 ** 32 - 16
    for family in ("across32", "across63", "top"):
        ids = FAMILIES[family](n)
        assert int(ids.max()) >= limit
        for order in ORDERS:
            with pytest.raises(vdb.VectorDbError) as e:
                h.build_batch((ids if order == "row" else ids[permutation(n)], rows))
            assert "2^32" in str(e.value)
            assert h.len() == 300
        for x in (int(ids[-1]), limit, 2 ** 32, 2 ** 63, 2 ** 64 - 1):
            with pytest.raises(vdb.VectorDbError):
                h.add(x, vdb.Vector(rows[0]))
            rc = h._L.vdb_hnsw_add(h._h, x, rows[0].ctypes.data_as(ctypes.POINTER(ctypes.c_float)), d, -1)
            assert rc == vdb._ffi.ERR_INVALID_ARGUMENT, rc
            assert h.len() == 300 and h.get_vector(x) is None and h.neighbors(x, 0) is None and h.level(x) < 0
            h.remove(x)                                                   # absent: Ok
            # a truncated id would have landed on a small one: (uint32) x names a stored node for none of these
            assert h.len() == 300
        # a batch whose LAST id is too large inserts nothing of its head either
        mixed = np.concatenate([small[300:310], ids[-1:]])
        with pytest.raises(vdb.VectorDbError):
            h.build_batch((mixed, rows[300:311]))
        assert h.len() == 300 and h.get_vector(int(small[300])) is None
    # ids == NULL: first_id + i.  A first_id at or above the limit is refused whatever follows, so a sum that wraps past 2^64 to a
    # small id is never reached; one that STARTS below the limit and runs into it is refused as a whole too
    fp = ctypes.POINTER(ctypes.c_float)
    for first in (2 ** 64 - 3, 2 ** 64 - 1, 2 ** 63, 2 ** 32, limit, limit - 2):
        rc = h._L.vdb_hnsw_add_bulk(h._h, None, first, rows[300:306].ctypes.data_as(fp), 6, d)
        assert rc == vdb._ffi.ERR_INVALID_ARGUMENT, (first, rc)
        held = {int(x) for x in small[:300]}
        assert h.len() == 300 and all(h.level((first + i) % 2 ** 64) < 0 for i in range(6) if (first + i) % 2 ** 64 not in held)
    # life goes on: add, remove and a re-add of ids it can hold, still the restatement's graph and results
    h.build_batch((small[300:], rows[300:]))
    for i in range(300, n):
        o.insert(int(small[i]), rows[i])
    for i in (5, 250, 399):
        h.remove(int(small[i]))
        o.remove(int(small[i]))
    h.add(int(small[250]), vdb.Vector(rows[7]))
    o.insert(int(small[250]), rows[7])
    assert h.len() == len(o)
    for i in (0, 100, 250, 398):
        assert h.neighbors(int(small[i]), 0) == o.neighbors(int(small[i]), 0), i
    mask_bits = int(small.max()) + 1
    on, mask = _mask(mask_bits, 6)
    on[:] = False
    on[small[::2].astype(np.int64)] = True
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    mask = np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64)
    hi, hd, hc = h.search_batch_arrays(q, 10, 40)
    mi, md, mc = h.search_batch_arrays(q, 10, 40, id_mask=mask, mask_bits=mask_bits)
    for b in range(8):
        oi, od = o.search(q[b], 10, 40)
        assert hc[b] == len(oi) and np.array_equal(hi[b, :hc[b]], oi) and np.array_equal(hd[b, :hc[b]].view(np.uint32), od.view(np.uint32)), b
        assert mc[b] > 0 and all(on[int(x)] for x in mi[b, :mc[b]])


# ------------------------------------------------------------------ the C++ host mirror
def test_cpp_host_mirror_carries_every_family(vdb):
    """tests/cpp/id_space_test.cpp: add / len / get_vector / search / remove / re-add by ids of every family through vdb_host.hpp
    (its ids are size_t); one tie group, so the printed order is the unsigned id order."""
    import subprocess
    exe = build_cpp_id_space_test(ROOT, vdb.build())
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "id space ok" in out.stdout, out.stderr + out.stdout
    got = {}
    for line in out.stdout.splitlines()[:-1]:
        fam, phase, *ids = line.split()
        got[fam, phase] = [int(x) for x in ids]
    n = 48
    for fam in FAMILIES:
        f = [int(x) for x in FAMILIES[fam](n)]
        left = [x for i, x in enumerate(f) if i % 3 and i != n - 1]
        assert got[fam, "first20"] == f[:20] and got[fam, "all"] == f, fam
        assert got[fam, "after_remove"] == left and got[fam, "readd"] == [f[-1]], fam
